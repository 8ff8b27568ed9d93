"""Host-side contract of the FP8 feed-forward mode (no GPU): what ctrlv_gemm_f8_serves accepts, the argument errors of the new
entry points, the mode setter of the plan, and the accuracy cost of the mode on the oracle (tests/f8_ref.py)."""
import ctypes

import pytest
import torch

from tests import f8_ref


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def lib(request):
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    return _lib.load(request.param)


def _desc(K, N=640, M=300, **kw):
    """A served feed-forward descriptor (fake, aligned addresses: the predicate is host code and dereferences nothing)."""
    from ctrlv_amd import _lib
    d = _lib.GemmDesc()
    d.A, d.W, d.out = 0x10000, 0x20000, 0x30000
    d.M, d.N, d.Cin, d.taps, d.mode = M, N, K, 1, 0
    d.lda, d.ldo, d.n_store = K, N, N
    d.s_acc = d.s1 = d.s2 = 1.0
    d.vdiv, d.vmod, d.vS = 1, 1 << 30, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_gemm_f8_serves(lib):
    serves = lambda d: lib.ctrlv_gemm_f8_serves(ctypes.byref(d))   # noqa: E731
    for K in (128, 640, 1280, 2560, 5120):
        assert serves(_desc(K)) == 1, K
    assert serves(_desc(320)) == 0                 # the C = 320 feed-forward keeps ff_fused
    assert serves(_desc(64)) == 0 and serves(_desc(192)) == 0
    assert serves(_desc(640, geglu=1, N=5120, ldo=2560, n_store=2560)) == 1
    assert serves(_desc(640, R1=0x40000, ldr1=640, R2=0x50000, ldr2=640)) == 1
    assert serves(_desc(640, V=0x60000, vmode=1, vdiv=16, vmod=3, ldv=640)) == 1
    assert serves(_desc(640, out_f32=1)) == 1
    # the split trunk (lo planes), the conv modes, a second A source
    assert serves(_desc(640, R1=0x40000, ldr1=640, R1_lo=0x70000)) == 0
    assert serves(_desc(640, R2=0x40000, ldr2=640, R2_lo=0x70000)) == 0
    assert serves(_desc(640, out_lo=0x70000)) == 0
    assert serves(_desc(640, mode=1, taps=9)) == 0
    assert serves(_desc(640, mode=2, taps=3)) == 0
    assert serves(_desc(640, A2=0x80000, lda2=640, c_split=320)) == 0
    # what the kernel does not do: SiLU, raw_out, n_scale2, N not a multiple of 32, pitches, GEGLU with a residual
    assert serves(_desc(640, act=1)) == 0
    assert serves(_desc(640, tile=1)) == serves(_desc(640, tile=2)) == 1 and serves(_desc(640, tile=5)) == 0
    assert serves(_desc(640, raw_out=0x90000, ld_raw=640)) == 0
    assert serves(_desc(640, n_scale2=32)) == 0
    assert serves(_desc(640, N=48, ldo=48, n_store=48)) == 0
    assert serves(_desc(640, lda=648)) == 0 and serves(_desc(640, lda=512)) == 0
    assert serves(_desc(640, lda=656)) == 1
    assert serves(_desc(640, A=0x10008)) == 0
    assert serves(_desc(640, geglu=1, N=5120, ldo=2560, n_store=2560, R1=0x40000, ldr1=2560)) == 0
    assert lib.ctrlv_gemm_f8_serves(None) == 0
    # a function of the layer's shape only
    assert serves(_desc(640, M=1)) == serves(_desc(640, M=115200)) == 1


def test_argument_errors_do_not_need_a_gpu(lib):
    from ctrlv_amd import _lib
    p8 = ctypes.c_void_p(0x1000)
    with pytest.raises(ValueError, match="non-null"):
        _lib.check(lib.ctrlv_gemm_f8(ctypes.byref(_lib.GemmDesc()), p8, p8, None), "ctrlv_gemm_f8", lib)
    with pytest.raises(ValueError, match="non-null"):
        _lib.check(lib.ctrlv_gemm_f8(ctypes.byref(_desc(640)), None, p8, None), "ctrlv_gemm_f8", lib)
    assert lib.ctrlv_gemm_f8(None, p8, p8, None) == -1
    # unserved descriptors: bad shape, before any HIP call
    for d in (_desc(320), _desc(640, mode=1, taps=9), _desc(640, out_lo=0x70000), _desc(640, A2=0x80000, lda2=640)):
        assert lib.ctrlv_gemm_f8(ctypes.byref(d), p8, p8, None) == -2
    with pytest.raises(ValueError, match="multiple of 128"):
        _lib.check(lib.ctrlv_gemm_f8(ctypes.byref(_desc(320)), p8, p8, None), "ctrlv_gemm_f8", lib)
    q = lambda *a: lib.ctrlv_quant_rows_f8(*a)   # noqa: E731
    x, s = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x3000)
    assert q(None, 4, 128, 128, None, None, 0.0, None, 1, 1, 0, p8, 128, s, None) == -1            # null x
    assert q(x, 4, 128, 128, p8, None, 1e-5, None, 1, 1, 0, p8, 128, s, None) == -1                # gamma without beta
    assert q(x, 4, 128, 128, None, None, 0.0, p8, 1, 1, 128, p8, 128, s, None) == -1               # V without LayerNorm
    assert q(x, 4, 132, 136, None, None, 0.0, None, 1, 1, 0, p8, 136, s, None) == -2               # K % 8
    assert q(x, 4, 5248, 5248, None, None, 0.0, None, 1, 1, 0, p8, 5248, s, None) == -2            # K > 5120
    assert q(x, 4, 128, 120, None, None, 0.0, None, 1, 1, 0, p8, 128, s, None) == -2               # ldx < K
    assert q(x, 4, 128, 128, None, None, 0.0, None, 1, 1, 0, p8, 100, s, None) == -2               # ldq < K
    assert q(x, 0, 128, 128, None, None, 0.0, None, 1, 1, 0, p8, 128, s, None) == -2               # no rows
    with pytest.raises(ValueError, match="row-vector"):
        _lib.check(q(x, 4, 128, 128, p8, p8, 1e-5, p8, 0, 1, 128, p8, 128, s, None), "ctrlv_quant_rows_f8", lib)


def test_plan_ff_precision_refuses_the_split_trunk():
    import __graft_entry__ as g
    g.build()
    from ctrlv_amd import _lib
    from ctrlv_amd.plan import config_struct
    import ctrlv_ref as R
    cfg = config_struct("unet", dict(R.TINY_CONFIG))
    lib16, libbf = _lib.load(torch.float16), _lib.load(torch.bfloat16)
    for lib in (lib16, libbf):
        h = ctypes.c_void_p()
        assert lib.ctrlv_plan_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
        assert lib.ctrlv_plan_set_ff_precision(h, 2) == -1 and lib.ctrlv_plan_set_ff_precision(None, 1) == -1
        assert lib.ctrlv_plan_set_ff_precision(h, 1) == 0        # (no weights loaded yet: nothing to quantise, no GPU needed)
        assert lib.ctrlv_plan_set_ff_precision(h, 1) == 0
        assert lib.ctrlv_plan_set_trunk_mode(h, 1) == -1         # either order: f8 first ...
        assert lib.ctrlv_plan_set_trunk_mode(h, 0) == 0
        assert lib.ctrlv_plan_set_ff_precision(h, 0) == 0
        if lib is lib16:
            assert lib.ctrlv_plan_set_trunk_mode(h, 1) == 0
            assert lib.ctrlv_plan_set_ff_precision(h, 1) == -1   # ... or the split trunk first
            with pytest.raises(ValueError, match="split trunk"):
                _lib.check(lib.ctrlv_plan_set_ff_precision(h, 1), "ctrlv_plan_set_ff_precision", lib)
            assert lib.ctrlv_plan_set_ff_precision(h, 0) == 0
        assert lib.ctrlv_plan_destroy(h) == 0


def test_model_attribute_is_validated():
    from ctrlv_amd.models.encoder import SpatioTemporalEncoderBase
    assert SpatioTemporalEncoderBase.ff_dtype in ("same", "f8")

    class M(SpatioTemporalEncoderBase):
        def __init__(self):
            pass
    m = M()
    m.ff_dtype = "f8"
    m._check_ff_dtype()
    m.trunk_dtype = "fp16x2"
    with pytest.raises(ValueError, match="fp16x2"):
        m._check_ff_dtype()
    m.trunk_dtype, m.ff_dtype = "same", "fp8"
    with pytest.raises(ValueError, match="ff_dtype"):
        m._check_ff_dtype()


def test_quant_rows_reference_contract():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 256, generator=g) * torch.tensor([1e-3, 1.0, 50.0, 1e4, 0.0]).unsqueeze(1)
    x[1, 7] = 3.0e38
    x[4] = 0.0
    q, s = f8_ref.quant_rows(x)
    codes = q.view(torch.uint8)
    assert s[4] == 1.0 and bool((codes[4] == 0).all())
    assert bool(((codes & 0x7f) != 0x7f).all())                                   # never a NaN code
    assert torch.equal(q.float().abs().amax(1)[:4], torch.full((4,), 448.0))      # each row's largest element is +-448
    assert torch.equal(s[:4], x[:4].abs().amax(1) / 448.0)
    # round-to-nearest: half an e4m3 ulp of the scaled value (3 mantissa bits; subnormal spacing 2^-9 below 2^-6)
    y = (x / s.unsqueeze(1)).abs()
    ulp = torch.exp2(torch.floor(torch.log2(y.clamp_min(2.0 ** -6))) - 3)
    assert bool(((q.float().abs() - y).abs() <= 0.5 * ulp * (1 + 1e-6)).all())


def test_fake_quantised_oracle_reproduces_the_predicted_cost():
    """The accuracy cost of the mode on TINY_CONFIG (B2 F3 16x16, bf16-rounded parameters): the 48 feed-forwards at C = 128 of
    the two models fake-quantised against the unquantised oracle -- rel-L2 7.2e-3 (UNet output), 1.6e-2 (mid residual),
    1.5e-2 (worst down residual), to two digits."""
    import ctrlv_ref as R
    from tests.parity_utils import make_inputs, oracle_forward
    cfg = dict(R.TINY_CONFIG)
    ou, oc = f8_ref.oracle_pair(cfg)
    qu, qc, n = f8_ref.quantised_copy(ou, oc)
    assert n == 48                                  # the C = 128 feed-forwards; the C = 64 ones are not served
    inp = make_inputs(cfg, 2, 3, 16, 16)
    e = f8_ref.errors(oracle_forward(qu, qc, inp, with_unet_no_ctrl=False), oracle_forward(ou, oc, inp, with_unet_no_ctrl=False))
    print(e)
    assert float(f"{e['unet']:.1e}") == 7.2e-3 and float(f"{e['mid']:.1e}") == 1.6e-2 and float(f"{e['down']:.1e}") == 1.5e-2, e
