"""Dynamic loss scaling of ctrlv_amd.optim without a GPU: the restatement of the device record's update
(tests/loss_scale_ref.py) against torch.amp.GradScaler on the CPU, the unscale formula, the two entry points in header, ctypes
table and both libraries, their host refusals, and the host side of `LossScaler` (state dict both ways, refusals, identity when
disabled, the keywords of the training steps)."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import loss_scale_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ctrlv_grad_finish_scaled", "ctrlv_adamw_step_scaled")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    return [_lib.load(torch.bfloat16), _lib.load(torch.float16)]


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_scaler_step(scaler, opt, p, found_inf):
    p.grad = torch.full_like(p, math.inf if found_inf else 1.0) * 1.0
    scaler.step(opt)
    scaler.update()


@pytest.mark.parametrize("name", sorted(L.SCRIPTS))
def test_restatement_against_torch_gradscaler(name):
    """scale and growth tracker equal torch's after EVERY step of a scripted finite / non-finite sequence."""
    script = L.SCRIPTS[name]
    rec = L.Record(**script["kw"])
    scaler = torch.amp.GradScaler("cpu", **script["kw"])
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=0.0)
    scaler.scale(torch.zeros(()))                           # (creates torch's scale tensor)
    seen = []
    for k, found in enumerate(script["found"]):
        skip = rec.step(found)
        _torch_scaler_step(scaler, opt, p, found)
        sd = scaler.state_dict()
        assert skip == int(found)
        assert rec.scale == sd["scale"] and rec.growth_tracker == sd["_growth_tracker"], (name, k, rec.scale, sd)
        seen.append((rec.scale, rec.growth_tracker))
    assert rec.skipped_total == sum(script["found"])
    scales = [s for s, _ in seen]
    if name == "interval3":
        s0 = L.f32(1000.0)
        assert scales[:3] == [s0, s0, L.f32(s0 * 3)] and seen[2][1] == 0          # growth exactly at the interval, not before
        assert seen[7][1] == 2 and seen[8] == (L.f32(scales[7] * 0.25), 0)         # the skip at tracker = interval - 1
        assert math.log2(s0) % 1 != 0.0
    if name == "overflow":
        assert scales[0] == scales[1] == L.f32(2.5e38) and seen[1][1] == 0         # growth refused, tracker reset all the same
        with np.errstate(over="ignore"):
            assert not math.isfinite(float(np.float32(2.5e38) * np.float32(3.0)))


def test_invalid_record_skips_and_keeps_its_scale():
    for bad in (0.0, -4.0, math.inf, math.nan):
        rec = L.Record(init_scale=1.0, growth_interval=1)
        rec.scale = bad
        assert rec.step(False) == 1 and rec.skipped_total == 1 and rec.growth_tracker == 0 and math.isnan(rec.unscale)
        assert rec.scale == bad or (math.isnan(bad) and math.isnan(rec.scale))


def test_unscale_formula_against_torch():
    """fp32(1 / (double)scale), then times grad_scale in fp32, for 1000 seeded scales."""
    gen = torch.Generator().manual_seed(11)
    scales = torch.exp2(torch.rand(1000, generator=gen) * 60.0 - 20.0).float()    # 2^-20 .. 2^40, not powers of two
    inv = scales.double().reciprocal().float()                                      # torch/amp/grad_scaler.py, unscale_
    for gs in (1.0, 0.25, 1.0 / 3.0):
        want = inv * torch.tensor(gs, dtype=torch.float32)
        got = [L.unscale(float(s), gs) for s in scales]
        assert got == want.tolist(), gs
    assert L.unscale(1024.0) == 2.0 ** -10 and L.unscale(3.0) == float(np.float32(1.0 / 3.0))


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_in_header_ctypes_and_both_libraries(libs):
    from ctrlv_amd import _lib
    text = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_int
        for lib in libs:
            assert getattr(lib, name) is not None
    assert re.search(r"typedef struct ctrlv_loss_scale_state\s*\{[^}]*\bscale;[^}]*\bunscale;[^}]*\bgrowth_tracker;[^}]*"
                     r"\bgrowth_interval;[^}]*\bgrowth_factor\s*,\s*backoff_factor;[^}]*\breserved\[2\];", hdr, flags=re.S)
    # the finish plus the record; the step without the grad_scale value, plus the record
    assert len(_lib.SIGNATURES["ctrlv_grad_finish_scaled"][1]) == len(_lib.SIGNATURES["ctrlv_grad_finish"][1]) + 1 == 7
    assert len(_lib.SIGNATURES["ctrlv_adamw_step_scaled"][1]) == len(_lib.SIGNATURES["ctrlv_adamw_step_dev"][1]) == 17
    assert _lib.ABI_VERSION == 22 and all(lib.ctrlv_abi_version() == 22 for lib in libs)        # additive: the number stays
    abi_comment = text[text.index("Library ABI version"):text.index("int ctrlv_abi_version")]
    for name in NAMES:
        assert name in abi_comment, name


def test_record_layout_is_32_bytes():
    from ctrlv_amd.optim import LossScaler
    s = LossScaler(init_scale=1000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)
    rec = s._record_on("cpu")
    assert rec.dtype == torch.int32 and rec.numel() == 8 and rec.numel() * rec.element_size() == 32
    f = rec.view(torch.float32)
    assert float(f[0]) == 1000.0 and float(f[1]) == 0.0 and int(rec[2]) == 0 and int(rec[3]) == 7
    assert float(f[4]) == 3.0 and float(f[5]) == 0.25 and rec[6:].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ host refusals
def _ptr(x):
    return ctypes.c_void_p(x) if x else None


@pytest.mark.parametrize("kw,match", [
    (dict(ls=0), "ls"), (dict(ls=0x40008), "ls"),
    # ... and ctrlv_grad_finish's own
    (dict(partials=0), "non-null"), (dict(state=0), "non-null"), (dict(count=0), "positive"), (dict(partials=0x20004), "aligned"),
    (dict(state=0x30008), "aligned"), (dict(max_norm=0.0), "max_norm"), (dict(max_norm=-1.0), "max_norm"),
    (dict(max_norm=math.nan), "max_norm"), (dict(max_norm=-math.inf), "max_norm"), (dict(grad_scale=math.inf), "grad_scale"),
    (dict(grad_scale=math.nan), "grad_scale"),
])
def test_finish_scaled_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    a = dict(dict(partials=0x20000, count=8, grad_scale=1.0, max_norm=1.0, ls=0x40000, state=0x30000), **kw)
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_grad_finish_scaled(_ptr(a["partials"]), a["count"], a["grad_scale"], a["max_norm"], _ptr(a["ls"]),
                                                    _ptr(a["state"]), None), "ctrlv_grad_finish_scaled", lib)


_OK = dict(p=0x10000, g=0x20000, m=0x30000, v=0x40000, ema=0x50000, n=1024, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2,
           bias1=0.1, bias2=0.001, ema_decay=0.999, ls=0x70000, state=0x60000)


@pytest.mark.parametrize("kw,match", [
    (dict(ls=0), "ls"), (dict(ls=0x70004), "ls"), (dict(state=0), "state"), (dict(state=0x60004), "state"),
    # ... and ctrlv_adamw_step's own, through the shared check
    (dict(p=0), "non-null"), (dict(g=0), "non-null"), (dict(n=0), "positive"), (dict(m=0x3000c), "aligned"), (dict(ema=0x50004), "aligned"),
    (dict(lr=math.nan), "lr"), (dict(beta1=1.0), "beta"), (dict(eps=0.0), "eps"), (dict(bias2=0.0), "bias"),
    (dict(ema_decay=1.5), "decay"),
])
def test_step_scaled_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    a = dict(_OK, **kw)
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_adamw_step_scaled(_ptr(a["p"]), _ptr(a["g"]), _ptr(a["m"]), _ptr(a["v"]), _ptr(a["ema"]), a["n"], a["lr"],
                                                   a["beta1"], a["beta2"], a["eps"], a["wd"], a["bias1"], a["bias2"], a["ema_decay"],
                                                   _ptr(a["ls"]), _ptr(a["state"]), None), "ctrlv_adamw_step_scaled", lib)


# ------------------------------------------------------------------------------------------------ the class
def _module():
    torch.manual_seed(1)
    m = torch.nn.Module()
    for i, shape in enumerate([(3,), (320, 3, 3), (7, 5)]):
        m.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(*shape)))
    return m


KW = dict(init_scale=1000.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=5)


def test_state_dict_has_torchs_keys_and_loads_into_gradscaler():
    from ctrlv_amd.optim import LossScaler
    mine = LossScaler(**KW)
    mine.scale(torch.ones(()))
    mine._rewrite(scale=750.0, tracker=3)                   # as if steps had run
    sd = mine.state_dict()
    theirs = torch.amp.GradScaler("cpu")
    assert set(sd) == set(theirs.state_dict()) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    theirs.load_state_dict(sd)
    theirs.scale(torch.ones(()))
    assert theirs.state_dict() == sd == dict(scale=750.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=5, _growth_tracker=3)


@pytest.mark.parametrize("record_first", [False, True])
def test_gradscaler_state_dict_loads_into_loss_scaler(record_first):
    from ctrlv_amd.optim import LossScaler
    theirs = torch.amp.GradScaler("cpu", **KW)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=0.0)
    theirs.scale(torch.zeros(()))
    for found in (False, False, True, False, False):
        _torch_scaler_step(theirs, opt, p, found)
    sd = theirs.state_dict()
    assert sd["scale"] == 250.0 and sd["_growth_tracker"] == 2
    mine = LossScaler()
    if record_first:
        mine.scale(torch.ones(()))
    mine.load_state_dict(sd)
    assert mine.state_dict() == sd
    assert float(mine.scale(torch.full((), 2.0))) == 500.0 and int(mine.growth_tracker_tensor()) == 2
    rec = mine._record_on("cpu")
    assert int(rec[3]) == 5 and rec.view(torch.float32)[4:6].tolist() == [3.0, 0.25]
    with pytest.raises(RuntimeError, match="empty"):
        mine.load_state_dict({})


def test_scale_multiplies_by_a_view_of_the_record():
    from ctrlv_amd.optim import LossScaler
    s = LossScaler(init_scale=2.0 ** 10)
    assert s.scale_tensor() is None and s.growth_tracker_tensor() is None and s.get_scale() == 1024.0
    loss = torch.tensor(0.5, requires_grad=True)
    out = s.scale(loss)
    assert float(out.detach()) == 512.0 and s.scale_tensor().dim() == 0 and s.scale_tensor().dtype == torch.float32
    assert s.scale_tensor().data_ptr() == s._record.data_ptr() and s.growth_tracker_tensor().data_ptr() == s._record.data_ptr() + 8
    out.backward()
    assert float(loss.grad) == 1024.0
    a, b = s.scale([torch.ones(()), torch.full((), 3.0)])
    assert float(a) == 1024.0 and float(b) == 3072.0
    s.update(new_scale=8.0)
    assert s.get_scale() == 8.0 and float(s.scale(torch.ones(()))) == 8.0


def test_step_raises_for_a_torch_optimiser():
    from ctrlv_amd.optim import AdamW, LossScaler
    m = _module()
    s = LossScaler()
    for opt in (torch.optim.AdamW(m.parameters()), torch.optim.SGD(m.parameters(), lr=0.1)):
        with pytest.raises(TypeError, match="AdamW"):
            s.step(opt)
    with pytest.raises(TypeError, match="LossScaler"):
        AdamW(_module().parameters()).step(scaler=torch.amp.GradScaler("cpu"))
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        s.unscale_(torch.optim.SGD(m.parameters(), lr=0.1))


def test_scaled_step_without_a_device_is_an_error_not_a_fallback():
    from ctrlv_amd import _lib
    from ctrlv_amd.optim import AdamW, LossScaler
    opt = AdamW(_module().parameters())
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):
        LossScaler().step(opt)
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):
        opt.step(scaler=LossScaler(), max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step(scaler=LossScaler(), max_grad_norm=0.0)


def test_disabled_is_the_identity():
    from ctrlv_amd.optim import LossScaler

    class Recording(torch.optim.SGD):
        calls = 0

        def step(self, closure=None):
            self.calls += 1
            return "stepped"

    s = LossScaler(enabled=False, growth_factor=0.5, backoff_factor=2.0)     # (not even validated, as in torch)
    loss = torch.tensor(0.5)
    assert s.scale(loss) is loss and s._record is None
    opt = Recording(_module().parameters(), lr=0.1)
    assert s.step(opt) == "stepped" and opt.calls == 1      # any optimiser, plain step()
    s.update()
    s.update(new_scale=4.0)
    assert s.get_scale() == 1.0 and s.state_dict() == {} and not s.is_enabled() and s._record is None
    s.load_state_dict({"scale": 3.0})                       # ignored
    assert s.get_scale() == 1.0
    with pytest.raises(ValueError, match="growth factor"):
        LossScaler(growth_factor=1.0)
    with pytest.raises(ValueError, match="backoff factor"):
        LossScaler(backoff_factor=1.0)


def test_training_steps_take_compute_dtype_and_scaler():
    from ctrlv_amd import training
    for fn in (training.train_step, training.unet_train_step):
        names = list(inspect.signature(fn).parameters)
        assert names[-3:] == ["max_grad_norm", "compute_dtype", "scaler"], fn.__name__
        assert all(inspect.signature(fn).parameters[k].default is None for k in names[-3:])
    assert "scaler" not in inspect.signature(training.vae_train_step).parameters


def test_a_scaler_needs_the_projects_optimiser():
    """`_backward_and_step` with a scaler and an optimiser that is not ours raises before the backward."""
    from ctrlv_amd.optim import LossScaler
    from ctrlv_amd.training import _backward_and_step
    m = _module()
    loss = sum((p * p).sum() for p in m.parameters())
    with pytest.raises(TypeError, match="AdamW"):
        _backward_and_step(m, loss, torch.optim.SGD(m.parameters(), lr=0.1), 1, None, False, 1.0, None, LossScaler())
    assert all(p.grad is None for p in m.parameters())
    # a disabled scaler is no scaler
    _backward_and_step(m, loss, torch.optim.SGD(m.parameters(), lr=0.1), 1, None, False, 1.0, None, LossScaler(enabled=False))


@pytest.mark.parametrize("bad", [torch.float32, torch.float64, torch.int8])
def test_compute_dtype_must_be_a_16_bit_float(bad):
    from ctrlv_amd import training
    with pytest.raises(ValueError, match="compute_dtype"):
        training._element_dtype(bad)
    assert training._element_dtype(None) is torch.bfloat16 and training._element_dtype(torch.float16) is torch.float16
