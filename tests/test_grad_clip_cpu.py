"""Global gradient-norm clipping of ctrlv_amd.optim.AdamW without a GPU: the three entry points (and the size query) in header,
ctypes table and both libraries, their host refusals, the argument check of `step(max_grad_norm=...)` ahead of any device work,
and the fp64 restatement (tests/grad_clip_ref.py) against torch.nn.utils.clip_grad_norm_ in double."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import grad_clip_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ctrlv_grad_sumsq", "ctrlv_grad_finish", "ctrlv_adamw_step_dev")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    return [_lib.load(torch.bfloat16), _lib.load(torch.float16)]


def _module():
    torch.manual_seed(1)
    m = torch.nn.Module()
    for i, shape in enumerate([(3,), (320, 3, 3), (7, 5)]):
        m.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(*shape)))
    return m


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
    assert re.search(r"\bsize_t\s+ctrlv_grad_sumsq_partials\s*\(", hdr)
    assert _lib.SIGNATURES["ctrlv_grad_sumsq_partials"][0] is ctypes.c_size_t
    assert re.search(r"typedef struct ctrlv_grad_state\s*\{[^}]*\bnorm;[^}]*\bcoef;[^}]*\bskip;[^}]*\bskipped_total;", hdr, flags=re.S)
    # ctrlv_adamw_step's arguments plus the record
    assert len(_lib.SIGNATURES["ctrlv_adamw_step_dev"][1]) == len(_lib.SIGNATURES["ctrlv_adamw_step"][1]) + 1 == 17
    assert _lib.ABI_VERSION == 22 and all(lib.ctrlv_abi_version() == 22 for lib in libs)        # additive: the number stays
    abi_comment = text[text.index("Library ABI version"):text.index("int ctrlv_abi_version")]
    for name in NAMES + ("ctrlv_grad_sumsq_partials",):
        assert name in abi_comment, name


def test_partition_is_a_function_of_n_alone(libs):
    for lib in libs:
        for n, want in ((1, 1), (4095, 1), (4096, 1), (4097, 2), (8191, 2), (8192, 2), (8193, 3), (680946897, 166247),
                        (2 ** 32 + 1, 2 ** 20 + 1)):
            assert lib.ctrlv_grad_sumsq_partials(n) == want == (n + G.BLOCK - 1) // G.BLOCK, n


# ------------------------------------------------------------------------------------------------ host refusals
def _ptr(x):
    return ctypes.c_void_p(x) if x else None


@pytest.mark.parametrize("kw,match", [
    (dict(g=0), "non-null"), (dict(partials=0), "non-null"), (dict(n=0), "positive"), (dict(g=0x10004), "aligned"),
    (dict(partials=0x20004), "aligned"),
    (dict(n=4097, length=1), "beyond"), (dict(n=4096, length=4, slot0=4), "beyond"), (dict(n=4096, length=4, slot0=5), "beyond"),
    (dict(n=4096, length=4, slot0=2 ** 64 - 1), "beyond"), (dict(n=8192, length=0), "beyond"),
])
def test_sumsq_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    a = dict(dict(g=0x10000, n=1024, partials=0x20000, length=8, slot0=0), **kw)
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_grad_sumsq(_ptr(a["g"]), a["n"], _ptr(a["partials"]), a["length"], a["slot0"], None),
                       "ctrlv_grad_sumsq", lib)


@pytest.mark.parametrize("kw,match", [
    (dict(partials=0), "non-null"), (dict(state=0), "non-null"), (dict(count=0), "positive"), (dict(partials=0x20004), "aligned"),
    (dict(state=0x30008), "aligned"), (dict(max_norm=0.0), "max_norm"), (dict(max_norm=-1.0), "max_norm"),
    (dict(max_norm=math.nan), "max_norm"), (dict(max_norm=-math.inf), "max_norm"), (dict(grad_scale=math.inf), "grad_scale"),
    (dict(grad_scale=math.nan), "grad_scale"),
])
def test_finish_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    a = dict(dict(partials=0x20000, count=8, grad_scale=1.0, max_norm=1.0, state=0x30000), **kw)
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_grad_finish(_ptr(a["partials"]), a["count"], a["grad_scale"], a["max_norm"], _ptr(a["state"]), None),
                       "ctrlv_grad_finish", lib)


_OK = dict(p=0x10000, g=0x20000, m=0x30000, v=0x40000, ema=0x50000, n=1024, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2,
           bias1=0.1, bias2=0.001, grad_scale=1.0, ema_decay=0.999, state=0x60000)


@pytest.mark.parametrize("kw,match", [
    (dict(state=0), "state"), (dict(state=0x60004), "state"),
    # ... and ctrlv_adamw_step's own, through the shared check
    (dict(p=0), "non-null"), (dict(g=0), "non-null"), (dict(n=0), "positive"), (dict(m=0x3000c), "aligned"), (dict(ema=0x50004), "aligned"),
    (dict(lr=math.nan), "lr"), (dict(beta1=1.0), "beta"), (dict(eps=0.0), "eps"), (dict(bias2=0.0), "bias"),
    (dict(grad_scale=math.inf), "grad_scale"), (dict(ema_decay=1.5), "decay"),
])
def test_step_dev_host_refusals(libs, kw, match):
    from ctrlv_amd import _lib
    a = dict(_OK, **kw)
    for lib in libs:
        with pytest.raises(ValueError, match=match):
            _lib.check(lib.ctrlv_adamw_step_dev(_ptr(a["p"]), _ptr(a["g"]), _ptr(a["m"]), _ptr(a["v"]), _ptr(a["ema"]), a["n"], a["lr"],
                                                a["beta1"], a["beta2"], a["eps"], a["wd"], a["bias1"], a["bias2"], a["grad_scale"],
                                                a["ema_decay"], _ptr(a["state"]), None), "ctrlv_adamw_step_dev", lib)


# ------------------------------------------------------------------------------------------------ the class
@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, -math.inf, 1e-60])
def test_step_validates_max_grad_norm_before_any_device_work(bad):
    """A ValueError, not the CtrlvHipError that CPU parameters earn: the argument is checked first (1e-60 is zero as an fp32)."""
    from ctrlv_amd.optim import AdamW
    opt = AdamW(_module().parameters())
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step(max_grad_norm=bad)
    assert all("step" not in opt.state[p] for g in opt.param_groups for p in g["params"])      # nothing was counted


@pytest.mark.parametrize("max_grad_norm", [1.0, math.inf])
def test_clipped_step_without_a_device_is_an_error_not_a_fallback(max_grad_norm):
    from ctrlv_amd import _lib
    from ctrlv_amd.optim import AdamW
    opt = AdamW(_module().parameters())
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):
        opt.step(max_grad_norm=max_grad_norm)
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):                                        # ... as the plain step
        opt.step()
    with pytest.raises(RuntimeError, match="grad_state"):
        opt.grad_state()


def test_training_steps_take_max_grad_norm():
    import inspect
    from ctrlv_amd import training
    for fn in (training.train_step, training.unet_train_step, training._backward_and_step):
        assert inspect.signature(fn).parameters["max_grad_norm"].default is None, fn.__name__


def test_clip_grad_norm_sets_the_default_of_step():
    """`vae_train_step` keeps its argument list (tests/test_vae_train_cpu.py pins it): its callers set the norm on the optimiser."""
    from ctrlv_amd import _lib
    from ctrlv_amd.optim import AdamW
    opt = AdamW(_module().parameters())
    assert opt.clip_grad_norm(1.0) is opt and opt._max_grad_norm == 1.0
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.clip_grad_norm(bad)
    assert opt._max_grad_norm == 1.0
    with pytest.raises(_lib.CtrlvHipError, match="GPU"):
        opt.step()
    assert opt.clip_grad_norm(None)._max_grad_norm is None


def test_other_optimisers_are_clipped_with_torchs_function():
    """`_backward_and_step` with an optimiser that is not ours: torch.nn.utils.clip_grad_norm_ in front of its step()."""
    from ctrlv_amd.training import _backward_and_step

    class Recording(torch.optim.SGD):
        def step(self):
            self.seen = [p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
            return super().step()

    out = {}
    for max_norm in (None, 1e-2):
        m = _module().double()
        opt = Recording(m.parameters(), lr=0.1)
        loss = sum((p * p).sum() for p in m.parameters())
        _backward_and_step(m, loss, opt, 1, None, False, 1.0, max_norm)
        out[max_norm] = opt.seen                                                               # the gradients its step() saw
    norm, coef, clipped = G.clip(out[None], 1e-2)
    assert coef < 1.0
    for got, want in zip(out[1e-2], clipped):
        assert torch.allclose(got, want, rtol=1e-12, atol=0.0)
    assert G.total_norm(out[1e-2]) == pytest.approx(1e-2 * norm / (norm + 1e-6), rel=1e-12)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("max_norm", [1.0, 1e-3, 1e6, math.inf])
@pytest.mark.parametrize("n", [1, 5, 257, 4099])
def test_restatement_agrees_with_torch_in_double(n, max_norm):
    _, grads = G.case(n)
    params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for _ in grads]
    for p, g in zip(params, grads):
        p.grad = g.double().clone()
    got = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef, clipped = G.clip(grads, max_norm)
    assert got == pytest.approx(norm, rel=1e-14, abs=0.0)
    assert 0.0 < coef <= 1.0 and (coef == 1.0) == (max_norm >= norm + 1e-6)
    for p, c in zip(params, clipped):
        assert torch.allclose(p.grad, c, rtol=1e-14, atol=0.0)
    # a scale in front: the norm is that of the scaled gradients
    assert G.total_norm(grads, 2.0 ** -7) == pytest.approx(norm * 2.0 ** -7, rel=1e-15)


def test_ulps_of():
    assert G.ulps_of(1.0, 1.0) == 0.0 and G.ulps_of(1.0 + 2.0 ** -23, 1.0) == 1.0 and G.ulps_of(3.0, 2.0) == 2.0 ** 22
    assert G.ulps_of(math.inf, 1.0) == math.inf and G.ulps_of(math.nan, 1.0) == math.inf and G.ulps_of(0.0, 0.0) == 0.0
