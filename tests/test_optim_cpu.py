"""ctrlv_amd.optim without a GPU: the EMA decay schedule, the flat layout of the AdamW parameter groups, torch's state-dict
layout, the host refusals of ctrlv_adamw_step / ctrlv_ema_step and the presence of the two symbols in header, ctypes and both
libraries."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    return [_lib.load(torch.bfloat16), _lib.load(torch.float16)]


# ------------------------------------------------------------------------------------------------ decay schedule
@pytest.mark.parametrize("kw", [dict(), dict(use_ema_warmup=True), dict(update_after_step=3),
                                dict(use_ema_warmup=True, update_after_step=3, inv_gamma=2.0, power=0.75),
                                dict(decay=0.95, min_decay=0.3)])
def test_decay_schedule(kw):
    from ctrlv_amd.optim import EMAModel, ema_decay_schedule
    ema = EMAModel([torch.nn.Parameter(torch.zeros(3))], **kw)
    for step in (0, 1, 2, 10, 10000):
        want = R.ema_decay(step, **kw)
        assert ema.get_decay(step) == pytest.approx(want, rel=1e-15, abs=0.0), (kw, step)
        assert ema_decay_schedule(step, **kw) == ema.get_decay(step)
    # values worked by hand from the schedule [DIFF-0.27.2, not in tree]
    if not kw:
        assert [ema.get_decay(s) for s in (0, 1)] == [0.0, 0.0]
        assert ema.get_decay(2) == pytest.approx(2 / 11) and ema.get_decay(10) == pytest.approx(10 / 19)
        assert ema.get_decay(10000) == pytest.approx(min(0.9999, 10000 / 10009))
    if kw == dict(use_ema_warmup=True):
        assert ema.get_decay(2) == pytest.approx(1 - 2 ** (-2 / 3)) and ema.get_decay(10) == pytest.approx(1 - 10 ** (-2 / 3))
    if kw == dict(update_after_step=3):
        assert [ema.get_decay(s) for s in (0, 1, 2, 4)] == [0.0] * 4 and ema.get_decay(10) == pytest.approx(7 / 16)
    if "min_decay" in kw:
        assert ema.get_decay(2) == 0.3 and ema.get_decay(10000) == 0.95 and ema.get_decay(1) == 0.0


def test_ema_fallback_on_cpu_follows_the_restatement():
    """Parameters outside a ctrlv optimiser: foreach ops on per-tensor shadows, diffusers' form (frozen parameters are copied)."""
    from ctrlv_amd.optim import EMAModel
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(7, 5)), torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(4), requires_grad=False)]
    ema = EMAModel(ps)
    ref = [p.detach().double().clone() for p in ps]
    for step in range(1, 6):
        with torch.no_grad():
            for p in ps:
                p.add_(0.1 * torch.randn_like(p))
        ema.step(ps)
        d = R.ema_decay(step)
        ref = [R.ema_step(r, p.detach().double(), d) if p.requires_grad else p.detach().double() for r, p in zip(ref, ps)]
        assert ema.optimization_step == step and ema.cur_decay_value == pytest.approx(d)
    for s, r, p in zip(ema.shadow_params, ref, ps):
        assert R.ulps(s, r, [p.detach()]) <= 4.0
    assert torch.equal(ema.shadow_params[2], ps[2].detach())
    # store / copy_to / restore: the parameters come back bit for bit
    before = [p.detach().clone() for p in ps]
    ema.store(ps)
    ema.copy_to(ps)
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, ema.shadow_params))
    ema.restore(ps)
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
    # state dict round trip
    other = EMAModel([torch.nn.Parameter(torch.zeros_like(p)) for p in ps])
    other.load_state_dict(ema.state_dict())
    assert other.optimization_step == 5 and all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))


# ------------------------------------------------------------------------------------------------ flat layout
def _module():
    torch.manual_seed(1)
    m = torch.nn.Module()
    for i, shape in enumerate([(1,), (3,), (320, 3, 3), (7, 5), (64,), (65,)]):
        m.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(*shape)))
    return m


def test_flat_layout_offsets_padding_and_groups():
    from ctrlv_amd.optim import ALIGN, AdamW
    m = _module()
    names = [n for n, _ in m.named_parameters()]
    values = [p.detach().clone() for p in m.parameters()]
    ids = [id(p) for p in m.parameters()]
    ps = list(m.parameters())
    opt = AdamW([{"params": ps[:4]}, {"params": ps[4:], "lr": 3e-4, "weight_decay": 0.0}], lr=1e-3)
    assert ALIGN == 64 and len(opt.param_groups) == 2
    assert [n for n, _ in m.named_parameters()] == names and [id(p) for p in m.parameters()] == ids     # same objects, same keys
    spans = []
    for gi, group in enumerate(opt.param_groups):
        pbuf, gbuf, mbuf, vbuf, offsets = opt.flat_buffers(gi)
        used = 0
        for p, off in zip(group["params"], offsets):
            assert off % 64 == 0
            assert p.data_ptr() == pbuf.data_ptr() + 4 * off and p.is_contiguous()
            assert p.grad is not None and p.grad.data_ptr() == gbuf.data_ptr() + 4 * off and p.grad.shape == p.shape
            spans.append((gi, off, off + p.numel()))
            used += p.numel()
        total = sum((p.numel() + 63) // 64 * 64 for p in group["params"])
        assert pbuf.numel() == gbuf.numel() == mbuf.numel() == vbuf.numel() == total            # padding is counted
        assert total - used == opt._flat[gi].padding
        mask = torch.zeros(total, dtype=torch.bool)
        for p, off in zip(group["params"], offsets):
            assert not bool(mask[off:off + p.numel()].any())                                     # no overlap
            mask[off:off + p.numel()] = True
        assert float(pbuf[~mask].abs().sum()) == 0.0 and float(mbuf.abs().sum()) == 0.0 and float(vbuf.abs().sum()) == 0.0
        assert all(b.data_ptr() % 16 == 0 for b in (pbuf, gbuf, mbuf, vbuf))
    assert opt.flat_buffers(0)[0].data_ptr() != opt.flat_buffers(1)[0].data_ptr()               # two groups, two buffers
    assert opt.flat_buffers(0)[0].numel() == 64 + 64 + 2880 + 64 and opt.flat_buffers(1)[0].numel() == 64 + 128
    assert all(torch.equal(p.detach(), v) for p, v in zip(m.parameters(), values))              # re-homing keeps the bits
    # autograd accumulates into the views; zero_grad keeps them whatever set_to_none says
    sum((p * p).sum() for p in m.parameters()).backward()
    gbuf = opt.flat_buffers(0)[1]
    assert torch.equal(ps[3].grad, 2 * ps[3].detach()) and ps[3].grad.data_ptr() == gbuf.data_ptr() + 4 * opt.flat_buffers(0)[4][3]
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is not None and float(p.grad.abs().sum()) == 0.0 for p in ps)
    assert float(gbuf.abs().sum()) == 0.0
    # add_param_group: a third buffer
    extra = torch.nn.Parameter(torch.randn(10))
    opt.add_param_group({"params": [extra]})
    assert len(opt.param_groups) == 3 and extra.data_ptr() == opt.flat_buffers(2)[0].data_ptr()
    with pytest.raises(ValueError):
        AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="already homed"):
        AdamW([extra])


def test_step_without_a_device_is_an_error_not_a_fallback():
    from ctrlv_amd import _lib
    from ctrlv_amd.optim import AdamW
    m = _module()
    opt = AdamW(m.parameters())
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):
        opt.step()


def test_state_dict_layout_is_torchs():
    from ctrlv_amd.optim import AdamW
    m, t = _module(), _module()
    groups = lambda mod: [{"params": list(mod.parameters())[:4], "lr": 2e-3}, {"params": list(mod.parameters())[4:], "weight_decay": 0.0}]  # noqa: E731
    ours, ref = AdamW(groups(m), lr=1e-3, betas=(0.8, 0.99), eps=1e-6), torch.optim.AdamW(groups(t), lr=1e-3, betas=(0.8, 0.99), eps=1e-6)
    a, b = ours.state_dict(), ref.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["state"] == b["state"] == {}
    # a torch checkpoint with state loads: the moments land in the flat buffers, the keys and types stay torch's
    for p in t.parameters():
        p.grad = torch.randn_like(p)
    ref.step()
    ours.load_state_dict(ref.state_dict())
    a, b = ours.state_dict(), ref.state_dict()
    assert a["param_groups"] == b["param_groups"] and sorted(a["state"]) == sorted(b["state"]) == list(range(6))
    for k in b["state"]:
        assert sorted(a["state"][k]) == sorted(b["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        assert float(a["state"][k]["step"]) == 1.0 and a["state"][k]["step"].dtype == b["state"][k]["step"].dtype
        assert torch.equal(a["state"][k]["exp_avg"], b["state"][k]["exp_avg"])
        assert torch.equal(a["state"][k]["exp_avg_sq"], b["state"][k]["exp_avg_sq"])
    mbuf, offsets = ours.flat_buffers(0)[2], ours.flat_buffers(0)[4]
    assert a["state"][2]["exp_avg"].data_ptr() == mbuf.data_ptr() + 4 * offsets[2]
    # ... and a checkpoint written here loads into torch's class
    back = torch.optim.AdamW(groups(_module()), lr=1e-3)
    back.load_state_dict(ours.state_dict())
    assert back.state_dict()["param_groups"] == b["param_groups"]
    assert torch.equal(back.state_dict()["state"][3]["exp_avg_sq"], b["state"][3]["exp_avg_sq"])


# ------------------------------------------------------------------------------------------------ host refusals, symbols
_OK = dict(p=0x10000, g=0x20000, m=0x30000, v=0x40000, ema=0x50000, n=1024, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2,
           bias1=0.1, bias2=0.001, grad_scale=1.0, ema_decay=0.999)


def _adamw(lib, **kw):
    a = dict(_OK, **kw)
    ptr = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return lib.ctrlv_adamw_step(ptr(a["p"]), ptr(a["g"]), ptr(a["m"]), ptr(a["v"]), ptr(a["ema"]), a["n"], a["lr"], a["beta1"], a["beta2"],
                                a["eps"], a["wd"], a["bias1"], a["bias2"], a["grad_scale"], a["ema_decay"], None)


@pytest.mark.parametrize("kw,match", [
    (dict(p=0), "non-null"), (dict(g=0), "non-null"), (dict(m=0), "non-null"), (dict(v=0), "non-null"),
    (dict(n=0), "positive"),
    (dict(p=0x10004), "aligned"), (dict(g=0x20008), "aligned"), (dict(m=0x3000c), "aligned"), (dict(v=0x40001), "aligned"),
    (dict(ema=0x50004), "aligned"),
    (dict(lr=math.inf), "lr"), (dict(lr=math.nan), "lr"),
    (dict(beta1=1.0), "beta"), (dict(beta1=-0.1), "beta"), (dict(beta2=1.0), "beta"), (dict(beta2=math.nan), "beta"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"),
    (dict(bias1=0.0), "bias"), (dict(bias1=1.5), "bias"), (dict(bias2=0.0), "bias"), (dict(bias2=math.nan), "bias"),
    (dict(ema_decay=1.5), "decay"), (dict(ema_decay=-0.1), "decay"), (dict(ema_decay=math.nan), "decay"),
])
def test_adamw_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(_adamw(lib, **kw), "ctrlv_adamw_step", lib)


@pytest.mark.parametrize("args,match", [((0, 0x10000, 64, 0.5), "non-null"), ((0x10000, 0, 64, 0.5), "non-null"),
                                        ((0x10000, 0x20000, 0, 0.5), "positive"), ((0x10004, 0x20000, 64, 0.5), "aligned"),
                                        ((0x10000, 0x20008, 64, 0.5), "aligned"), ((0x10000, 0x20000, 64, 1.5), "decay"),
                                        ((0x10000, 0x20000, 64, -0.5), "decay"), ((0x10000, 0x20000, 64, math.nan), "decay")])
def test_ema_host_refusals(libs, args, match):
    from ctrlv_amd import _lib
    e, p, n, d = args
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_ema_step(ctypes.c_void_p(e) if e else None, ctypes.c_void_p(p) if p else None, n, d, None),
                       "ctrlv_ema_step", lib)


def test_symbols_in_header_ctypes_and_both_libraries(libs):
    import __graft_entry__ as g
    from ctrlv_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read(), flags=re.S)
    assert "optim.hip" in g.HIP_SOURCES
    for name in ("ctrlv_adamw_step", "ctrlv_ema_step"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
        for lib in libs:
            assert getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["ctrlv_adamw_step"][1]) == 16 and len(_lib.SIGNATURES["ctrlv_ema_step"][1]) == 5
