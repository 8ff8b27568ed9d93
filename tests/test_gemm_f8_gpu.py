"""GPU tests of the FP8 feed-forward kernels (csrc/quant_f8.hip, csrc/gemm_f8.hip) through ops, in both element libraries.

1. EXACT lane maps: small-integer operands (exact in e4m3 and in the fp32 accumulator) against the int64 product, bit for bit --
   decides the operand byte order of v_mfma_scale_f32_32x32x64_f8f6f4, cbsz = blgp = 0 and the unit block scales.
2. Scales and epilogues against fp64 on the same codes and scales (tests/f8_ref.py): the only error sources are the fp32
   summation order and one 16-bit rounding, so the bound is the one of the 16-bit GEMM tests -- parity_err < 3e-3 with bf16
   elements, a sixth of it with fp16 elements (tests/test_ops_gpu.py `tol`).
3. ctrlv_quant_rows_f8 by properties (a tie in fp32 cannot fail them).
4. One feed-forward through the four launches against the CPU computation on f8_ref-quantised operands, same bound, each half
   on the 16-bit operands the device itself stored (test_feed_forward_pair says why).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import f8_ref
from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def el(request, hip_lib):
    return request.param


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


def tol(el, bf16_bound=3e-3):
    return bf16_bound if el == torch.bfloat16 else bf16_bound / 6.0


def g(seed):
    return torch.Generator().manual_seed(seed)


def codes(q):
    """e4m3 tensor -> its bytes on the device"""
    return q.view(torch.uint8).contiguous().to(DEV)


def geglu_ref(lin):
    """GEGLU over packed columns: 16-column (value | gate) blocks -> [M, N / 2]"""
    M, N = lin.shape
    b = lin.reshape(M, N // 32, 2, 16)
    return (b[:, :, 0] * F.gelu(b[:, :, 1])).reshape(M, N // 2)


# ------------------------------------------------------------------------------------------------ 1. exact lane maps
@pytest.mark.parametrize("M,N,K", [(64, 64, 128), (200, 96, 384), (333, 640, 640), (1000, 256, 2560)])
def test_exact_integer_product(ops, el, M, N, K):
    A = torch.randint(-2, 3, (M, K), generator=g(M + K))
    W = torch.randint(-2, 3, (N, K), generator=g(N + K + 1))
    ref = (A @ W.T).float()                                   # int64 product, |.| <= 4 K: exact in fp32
    Ad, Wd = codes(A.float().to(torch.float8_e4m3fn)), codes(W.float().to(torch.float8_e4m3fn))
    ones_m, ones_n = torch.ones(M, device=DEV), torch.ones(N, device=DEV)
    out = torch.full((M, N), float("nan"), device=DEV)
    assert ops.gemm_f8_serves(Ad, Wd, out, N=N, cin=K, out_f32=True, el=el)
    ops.gemm_f8(Ad, ones_m, Wd, ones_n, out, N=N, cin=K, out_f32=True, el=el)
    got = out.cpu()
    bad = (got != ref).nonzero()
    print(f"exact {M}x{N}x{K}: {bad.shape[0]} elements differ" + (f", first {bad[:4].tolist()}" if bad.shape[0] else ""))
    assert torch.equal(got, ref)
    # a wider pitch of A reads the same values; n_store keeps the columns behind it untouched
    Aw = torch.full((M, K + 64), 0x7f, dtype=torch.uint8, device=DEV)       # (NaN codes in the gap: must never be read)
    Aw[:, :K] = Ad
    out2 = torch.full((M, N), -7.0, device=DEV)
    ops.gemm_f8(Aw[:, :K], ones_m, Wd, ones_n, out2, N=N, cin=K, out_f32=True, n_store=N - 32, el=el)
    assert torch.equal(out2[:, :N - 32].cpu(), ref[:, :N - 32]) and bool((out2[:, N - 32:] == -7.0).all())


@pytest.mark.parametrize("M,N,K", [(333, 640, 640), (600, 288, 256)])
def test_exact_integer_product_on_the_256_tile(ops, el, M, N, K):
    """The 256 x 256 tile (what large launches run on), forced at sizes ragged in both dimensions."""
    A = torch.randint(-2, 3, (M, K), generator=g(M + K))
    W = torch.randint(-2, 3, (N, K), generator=g(N + K + 1))
    ref = (A.double() @ W.double().T).float()
    Ad, Wd = codes(A.float().to(torch.float8_e4m3fn)), codes(W.float().to(torch.float8_e4m3fn))
    out = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_f8(Ad, torch.ones(M, device=DEV), Wd, torch.ones(N, device=DEV), out, N=N, cin=K, out_f32=True, el=el, tile=2)
    assert torch.equal(out.cpu(), ref)


def test_tile_choice_changes_no_bit(ops, el):
    """A launch large enough for the 256 x 256 tile (chosen by size) against the 128 x 128 tile forced, and a row block of it
    computed alone: the same bits -- 16-bit output with scales, bias and a residual, and GEGLU."""
    M, N, K = 4000, 4096, 256
    A = torch.randn(M, K, generator=g(21)) * (1.0 + torch.arange(M).float().unsqueeze(1) % 3)
    W = torch.randn(N, K, generator=g(22)) / math.sqrt(K)
    (qa, sa), (qw, sw) = f8_ref.quant_rows(A), f8_ref.quant_rows(W)
    qa, sa, qw, sw = codes(qa), sa.to(DEV), codes(qw), sw.to(DEV)
    bias, R1 = torch.randn(N, generator=g(23)).to(DEV), torch.randn(M, N, generator=g(24)).to(el).to(DEV)
    outs = []
    for tile in (0, 1, 2):
        o = torch.empty(M, N, dtype=el, device=DEV)
        ops.gemm_f8(qa, sa, qw, sw, o, N=N, cin=K, bias=bias, R1=R1, s1=0.5, tile=tile)
        u = torch.empty(M, N // 2, dtype=el, device=DEV)
        ops.gemm_f8(qa, sa, qw, sw, u, N=N, cin=K, bias=bias, geglu=1, tile=tile)
        outs.append((o, u))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0])
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][1], outs[2][1])
    part = torch.empty(300, N, dtype=el, device=DEV)
    ops.gemm_f8(qa[500:800], sa[500:800], qw, sw, part, N=N, cin=K, bias=bias, R1=R1[500:800], s1=0.5)
    assert torch.equal(part, outs[0][0][500:800])
    lin = (qa[:64].cpu().view(torch.float8_e4m3fn).double() @ qw.cpu().view(torch.float8_e4m3fn).double().T) \
        * sa[:64].cpu().double().unsqueeze(1) * sw.cpu().double().unsqueeze(0) + bias.cpu().double() + 0.5 * R1[:64].cpu().double()
    assert parity_err(outs[0][0][:64], lin.float(), what="256 tile, first rows") < tol(el)


# ------------------------------------------------------------------------------------------------ 2. scales and epilogues
@pytest.fixture(scope="module")
def epi_case():
    """Operands and fp64 products of the three shapes, made once"""
    cache = {}

    def get(M, N, K):
        if (M, N, K) not in cache:
            A = torch.randn(M, K, generator=g(1)) * (1.0 + torch.arange(M).float().unsqueeze(1) % 7)
            W = torch.randn(N, K, generator=g(2)) / math.sqrt(K) * (0.5 + torch.arange(N).float().unsqueeze(1) % 5)
            qa, sa = f8_ref.quant_rows(A)
            qw, sw = f8_ref.quant_rows(W)
            lin = (qa.double() @ qw.double().T) * sa.double().unsqueeze(1) * sw.double().unsqueeze(0)
            cache[(M, N, K)] = dict(qa=codes(qa), sa=sa.to(DEV), qw=codes(qw), sw=sw.to(DEV), lin=lin,
                                    bias=torch.randn(N, generator=g(3)), R1=torch.randn(M, N, generator=g(4)),
                                    R2=torch.randn(M, N, generator=g(5)), V=torch.randn(7, N, generator=g(6)))
        return cache[(M, N, K)]
    return get


@pytest.mark.parametrize("M,N,K", [(200, 256, 128), (333, 1280, 640), (72, 640, 2560)])
def test_scales_and_epilogues(ops, el, epi_case, M, N, K):
    c = epi_case(M, N, K)
    qa, sa, qw, sw = c["qa"], c["sa"], c["qw"], c["sw"]
    bias, V = c["bias"], c["V"]
    R1, R2 = c["R1"].to(el), c["R2"].to(el)
    lin = c["lin"] + bias.double()
    bd, Vd, R1d, R2d = bias.to(DEV), V.to(DEV), R1.to(DEV), R2.to(DEV)
    vidx = (torch.arange(M) // 13) % 7
    out = torch.empty(M, N, dtype=el, device=DEV)

    def run(o=out, A=qa, **kw):
        ops.gemm_f8(A, sa, qw, sw, o, N=N, cin=K, **kw)
        return o

    def check(got, ref, what):
        e = parity_err(got, ref.float(), what=f"{what} {M}x{N}x{K}")
        assert e < tol(el), (what, e)

    check(run(bias=bd), lin, "bias")
    check(run(), c["lin"], "plain")
    check(run(bias=bd, R1=R1d, s1=0.5, s_acc=0.7), 0.7 * lin + 0.5 * R1.double(), "R1 s1 s_acc")
    check(run(bias=bd, R1=R1d, s1=0.5, R2=R2d, s2=-0.25, s_acc=0.7), 0.7 * lin + 0.5 * R1.double() - 0.25 * R2.double(), "R1 + R2")
    check(run(bias=bd, R1=R1d, V=Vd, vmode=1, vdiv=13, vmod=7), lin + R1.double() + V[vidx].double(), "V vmode 1")
    # GEGLU: bias only, N / 2 output columns
    ug = torch.empty(M, N // 2, dtype=el, device=DEV)
    check(run(ug, bias=bd, geglu=1), geglu_ref(lin), "geglu")
    # fp32 output: only the summation order is left
    of = torch.empty(M, N, device=DEV)
    ops.gemm_f8(qa, sa, qw, sw, of, N=N, cin=K, bias=bd, out_f32=True, el=el)
    assert parity_err(of, lin.float(), what="fp32 out") < 1e-4
    # a second run gives the same bits; a wider lda reads the same values
    first = run(bias=bd, R1=R1d, s1=0.5, R2=R2d, s2=-0.25, s_acc=0.7).clone()
    assert torch.equal(run(bias=bd, R1=R1d, s1=0.5, R2=R2d, s2=-0.25, s_acc=0.7), first)
    Aw = torch.full((M, K + 48), 0x7f, dtype=torch.uint8, device=DEV)
    Aw[:, :K] = qa
    assert torch.equal(run(A=Aw[:, :K], bias=bd, R1=R1d, s1=0.5, R2=R2d, s2=-0.25, s_acc=0.7), first)


# ------------------------------------------------------------------------------------------------ 3. quant_rows_f8
def _e4m3_ulp(v):
    """spacing of e4m3 at |v| <= 448 (3 mantissa bits; subnormal spacing 2^-9 below 2^-6)"""
    return torch.exp2(torch.floor(torch.log2(v.clamp_min(2.0 ** -6))) - 3)


def _check_quant(q, s, y, exact_scale):
    """the properties of the contract, device codes / scales against the fp32 CPU value y"""
    qf = q.cpu().view(torch.float8_e4m3fn).float()
    s = s.cpu()
    byte = q.cpu()
    assert bool(((byte & 0x7f) != 0x7f).all()), "NaN code"
    a = y.abs().amax(1)
    want = torch.where(a > 0, a / 448.0, torch.ones_like(a))
    if exact_scale:
        assert torch.equal(s, want)
    else:
        assert bool(((s - want).abs() <= 1e-5 * want).all()), ((s - want).abs() / want).max()
    nz = a > 0
    assert torch.equal(qf.abs().amax(1)[nz], torch.full((int(nz.sum()),), 448.0))
    assert bool((byte[~nz] == 0).all()) and bool((s[~nz] == 1.0).all())
    su = s.unsqueeze(1)
    lim = su * (0.5 * _e4m3_ulp(y.abs() / su) + 2.0 ** -10)
    err = (qf * su - y).abs()
    worst = (err / lim).max().item()
    print(f"  quant property: worst |q s - y| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("M,K", [(7, 128), (333, 640), (64, 5120)])
def test_quant_rows_f8(ops, el, M, K):
    x = (torch.randn(M, K, generator=g(K)) * (0.01 + torch.arange(M).float().unsqueeze(1) % 5)).to(el)
    x[M // 2] = 0                                               # an all-zero row
    x[0, K - 1] = torch.finfo(el).max                           # the element type's largest finite value
    x[1, 3] = -torch.finfo(el).max
    xd = x.to(DEV)
    # plain: the scale is bit-exact (one IEEE division)
    q, s = ops.quant_rows_f8(xd)
    _check_quant(q, s, x.float(), exact_scale=True)
    # a wider output pitch writes the same codes and leaves the gap alone
    qw = torch.full((M, K + 24), 0x55, dtype=torch.uint8, device=DEV)
    ops.quant_rows_f8(xd, qw[:, :K], torch.empty(M, device=DEV))
    assert torch.equal(qw[:, :K], q) and bool((qw[:, K:] == 0x55).all())
    # LayerNorm folded in, without and with the row-vector add: fp32 statistics, the value never rounded to 16 bits
    x2 = (torch.randn(M, K, generator=g(K + 1)) * 3 + 0.5).to(el)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g(7)), 0.1 * torch.randn(K, generator=g(8))
    V = torch.randn(3, K, generator=g(9))
    for Vt in (None, V):
        xin = x2.float() + (V[(torch.arange(M) // 2) % 3] if Vt is not None else 0.0)
        y = F.layer_norm(xin, (K,), gamma, beta, 1e-5)
        q, s = ops.quant_rows_f8(x2.to(DEV), ln=(gamma.to(DEV), beta.to(DEV), 1e-5), V=None if Vt is None else Vt.to(DEV),
                                 vdiv=2, vmod=3)
        _check_quant(q, s, y, exact_scale=False)


# ------------------------------------------------------------------------------------------------ 4. pair against pair
@pytest.mark.parametrize("C", [128, 640])
def test_feed_forward_pair(ops, el, C):
    """LayerNorm + quantise, GEGLU projection, quantise u, output projection + bias + residual: the four launches of
    blocks._ln_ff / plan.hip ln_ff against the same chain on the CPU with tests/f8_ref.py.

    Each half is held to the bound: u against the CPU chain from x, the output against the CPU chain from the u THE DEVICE
    STORED.  Chaining the CPU's own u into the second half instead makes the comparison depend on ties: the device's GEGLU
    (tabulated Phi, |error| <= 1.2e-5) and the CPU's erf round a fraction of a percent of the u elements to neighbouring 16-bit
    values, and a 16-bit neighbour lands on the other e4m3 code with probability 2^-8 / 2^-3.5 (bf16) -- a handful of flipped
    codes of 1/16 relative size each, which no kernel can avoid and which alone measure 5.1e-3 on the element-wise part of
    parity_err at C = 128 in bf16 (rel-L2 1.8e-3; bound 3e-3) and 2.5e-3 / 2.2e-3 at C = 128 / 640 in fp16 (rel-L2 5.1e-4 /
    7.4e-4; bound 5e-4), where the two halves on identical operands measure 3.2e-4 and 1.3e-4; that figure is printed, not
    asserted."""
    from ctrlv_amd import packing
    M = 300
    x = (torch.randn(M, C, generator=g(10)) * 2 + 0.3).to(el)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g(11)), 0.1 * torch.randn(C, generator=g(12))
    w1 = (torch.randn(8 * C, C, generator=g(13)) / math.sqrt(C)).to(el)
    b1 = 0.1 * torch.randn(8 * C, generator=g(14))
    w2 = (torch.randn(C, 4 * C, generator=g(15)) / math.sqrt(4 * C)).to(el)
    b2 = 0.1 * torch.randn(C, generator=g(16))
    R1 = torch.randn(M, C, generator=g(17)).to(el)
    # CPU: the contract on the unpacked weights
    ya = f8_ref.fake_quant(F.layer_norm(x.float(), (C,), gamma, beta, 1e-5))
    h, gate = (ya.double() @ f8_ref.fake_quant(w1.float()).double().T + b1.double()).chunk(2, dim=-1)
    u = (h * F.gelu(gate)).float().to(el)                       # u is stored in the element type
    w2q = f8_ref.fake_quant(w2.float()).double()
    ref_chain = f8_ref.fake_quant(u.float()).double() @ w2q.T + b2.double() + R1.double()
    # device: packed weights (GEGLU rows interleaved), quantised by the same entry point
    with packing.element_dtype(el):
        w1p, b1p = packing.pack_geglu(w1, b1)
        w2p = packing.pack_linear(w2)
    q1w, s1w = ops.quant_rows_f8(w1p.to(DEV))
    q2w, s2w = ops.quant_rows_f8(w2p.to(DEV))
    q = torch.empty(M * 4 * C, dtype=torch.uint8, device=DEV)
    qs = torch.empty(M, device=DEV)
    qa, qu = q[:M * C].view(M, C), q.view(M, 4 * C)
    ud = torch.empty(M, 4 * C, dtype=el, device=DEV)
    out = torch.empty(M, C, dtype=el, device=DEV)
    R1d = R1.to(DEV)
    ops.quant_rows_f8(x.to(DEV), qa, qs, ln=(gamma.to(DEV), beta.to(DEV), 1e-5))
    ops.gemm_f8(qa, qs, q1w, s1w, ud, N=8 * C, cin=C, bias=b1p.to(DEV), geglu=1)
    e_u = parity_err(ud, u.float(), what=f"u C={C}")
    ops.quant_rows_f8(ud, qu, qs)
    ops.gemm_f8(qu, qs, q2w, s2w, out, N=C, cin=4 * C, bias=b2.to(DEV), R1=R1d)
    # the second half on the u the device stored: both sides quantise the SAME 16-bit values (see the docstring)
    ref = f8_ref.fake_quant(ud.cpu().float()).double() @ w2q.T + b2.double() + R1.double()
    e = parity_err(out, ref.float(), what=f"ff pair C={C}")
    parity_err(out, ref_chain.float(), what=f"ff pair C={C} against the CPU's own u (code flips included)")
    assert e_u < tol(el) and e < tol(el), (e_u, e)
