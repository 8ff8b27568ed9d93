"""First slice of the training path (BASELINE config 5; reference: tools/train_video_controlnet.py:451-488): backward of
the gather-GEMM family, GroupNorm(+SiLU) and a complete SpatioTemporalResBlock / ControlNet zero-conv through the HIP
kernels (ctrlv_amd/autograd.py, csrc/backward.hip), against torch.autograd.

Tolerances.  Kernel level (fp32 outputs from bf16 inputs, fp32 accumulation): rel-L2 <= 2e-3 against an fp32 reference on
the same bf16-rounded operands (the weight-gradient contraction runs over up to ~10^4 rows; atomics make the summation
order vary run to run within this bound).  Block level: gradients travel through eight bf16-stored activation gradients
and the forward's bf16 activations, against the oracle's fp32 autograd: rel-L2 <= 3e-2 (measured values are printed).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def g(seed):
    return torch.Generator().manual_seed(seed)


def bf(x):
    return x.to(torch.bfloat16)


def rows(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def nchw(r, n, h, w):
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.mark.parametrize("M,N,K", [(1000, 128, 64), (4096, 320, 320), (777, 64, 128)])
def test_wgrad_linear_and_colsum(ops, M, N, K):
    A, dY = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(M, N, generator=g(2)))
    dW = torch.zeros(N, K, dtype=torch.float32, device=DEV)
    dbf = torch.zeros(N, dtype=torch.float32, device=DEV)
    ops.gemm_wgrad(A.to(DEV), dY.to(DEV), dW, N=N, cin=K, dbias=dbf, scale=0.75)      # fused bias gradient + scale
    assert parity_err(dW, 0.75 * dY.float().T @ A.float(), "linear wgrad") < 2e-3
    assert parity_err(dbf, 0.75 * dY.float().sum(0), "fused bias grad") < 2e-3
    db = torch.zeros(N, dtype=torch.float32, device=DEV)
    ops.colsum(dY.to(DEV), db, scale=0.5)
    assert parity_err(db, 0.5 * dY.float().sum(0), "bias grad") < 2e-3
    dV = torch.zeros(3, N, dtype=torch.float32, device=DEV)
    vdiv = (M + 2) // 3
    ops.colsum(dY.to(DEV), dV, vmode=1, vdiv=vdiv, vmod=3)
    ref = torch.stack([dY.float()[i * vdiv:(i + 1) * vdiv].sum(0) for i in range(3)])
    assert parity_err(dV, ref, "row-vector grad") < 2e-3


@pytest.mark.parametrize("M,N,K,taps", [(20000, 320, 320, 1), (9000, 128, 64, 9), (50000, 64, 64, 1)])
def test_parameter_gradient_reductions_are_bit_reproducible(ops, M, N, K, taps):
    """wgrad (incl. the fused bias gradient and the [N][Cin][taps] scatter), colsum (bias and per-clip row-vector form) and
    dot_diff: slab / block partials added in a fixed order -- the same bits in every run (the atomics of
    the one-kernel forms arrive in a different order every time), and the same values as the atomic forms."""
    assert ops.DETERMINISTIC
    H = W = 0
    if taps == 9:
        n, H, W = 3, 50, 60
        M = n * H * W
    A, dY = bf(torch.randn(M, K, generator=g(1))).to(DEV), bf(torch.randn(M, N, generator=g(2))).to(DEV)
    kw = dict(N=N, cin=K, taps=taps, mode=1 if taps == 9 else 0, conv=(H, W, H, W, 1, 0) if taps == 9 else None)

    def grads(torch_layout):
        dW = torch.zeros(N, K, taps, dtype=torch.float32, device=DEV) if torch_layout else torch.zeros(N, taps * K, dtype=torch.float32, device=DEV)
        db = torch.zeros(N, dtype=torch.float32, device=DEV)
        for _ in range(2):                                      # accumulates: two calls into the same buffers
            ops.gemm_wgrad(A, dY, dW, dbias=db, scale=0.5, torch_layout=torch_layout, **kw)
        dV = torch.zeros(4, N, dtype=torch.float32, device=DEV)
        ops.colsum(dY, dV, vmode=1, vdiv=1024, vmod=4)
        acc = torch.zeros(1, dtype=torch.float32, device=DEV)
        ops.dot_diff(dY, dY, A[:, :N].contiguous() if K >= N else dY, acc, scale=0.25)
        return dW, db, dV, acc
    runs = [grads(tl) for tl in (False, False, False, True, True)]
    for r in runs[1:3]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[4], runs[3]))
    if taps > 1:                                                # the parameter's own layout = the packed one, permuted
        assert torch.equal(runs[3][0], runs[0][0].reshape(N, taps, K).permute(0, 2, 1).contiguous())
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, False
    try:
        ref = grads(False)
    finally:
        ops.DETERMINISTIC = prev
    for a, b in zip(runs[0], ref):
        assert parity_err(a, b) < 1e-4


@pytest.mark.parametrize("M", [1, 2, 3, 65, 66, 259, 1027])
def test_colsum_deterministic_with_blocks_of_fewer_than_four_rows(ops, M):
    """the ordered colsum dropped rows when a block held fewer than four rows (M < 4, or a last block of
    1-3 rows: row lanes without rows kept the 'no table row' mark, the fold was skipped and the lanes' plain stores overwrote
    each other).  Bias form and per-clip row-vector form, against fp32 torch and against the atomic form."""
    assert ops.DETERMINISTIC
    N = 72
    dY = bf(torch.randn(M, N, generator=g(M))).to(DEV)

    def run():
        db = torch.zeros(N, dtype=torch.float32, device=DEV)
        ops.colsum(dY, db, scale=0.5)
        dV = torch.zeros(1, N, dtype=torch.float32, device=DEV)
        ops.colsum(dY, dV, vmode=1, vdiv=1 << 20, vmod=1)          # (M = B rows of a per-clip GEMM: one table row)
        return db, dV
    db, dV = run()
    ref = dY.float().sum(0)
    assert parity_err(db, 0.5 * ref, "bias grad, ragged blocks") < 1e-5
    assert parity_err(dV[0], ref, "row-vector grad, ragged blocks") < 1e-5
    prev, ops.DETERMINISTIC = ops.DETERMINISTIC, False
    try:
        db_a, dV_a = run()
    finally:
        ops.DETERMINISTIC = prev
    assert parity_err(db, db_a) < 1e-5 and parity_err(dV, dV_a) < 1e-5
    db2, dV2 = run()
    assert torch.equal(db, db2) and torch.equal(dV, dV2)


@pytest.mark.parametrize("stride,up", [(1, 0), (2, 0), (1, 1)])
def test_wgrad_conv3x3(ops, stride, up):
    n, cin, cout, H, W = 3, 64, 128, 12, 10
    x = bf(torch.randn(n, cin, H, W, generator=g(1)))
    Ho, Wo = ((H << up) + 2 - 3) // stride + 1, ((W << up) + 2 - 3) // stride + 1
    dy = bf(torch.randn(n, cout, Ho, Wo, generator=g(2)))
    w = torch.zeros(cout, cin, 3, 3, requires_grad=True)
    xin = x.float()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    F.conv2d(xin, w, None, stride=stride, padding=1).backward(dy.float())
    dW = torch.zeros(cout, 9 * cin, dtype=torch.float32, device=DEV)
    ops.gemm_wgrad(rows(x).to(DEV), rows(dy).to(DEV), dW, N=cout, cin=cin, taps=9, mode=1, conv=(H, W, Ho, Wo, stride, up))
    got = dW.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    assert parity_err(got, w.grad, f"conv3x3 wgrad stride {stride} up {up}") < 2e-3
    dWt = torch.zeros(cout, cin, 3, 3, dtype=torch.float32, device=DEV)       # the parameter's own layout
    ops.gemm_wgrad(rows(x).to(DEV), rows(dy).to(DEV), dWt, N=cout, cin=cin, taps=9, mode=1, conv=(H, W, Ho, Wo, stride, up),
                   torch_layout=True)
    assert parity_err(dWt, w.grad, "conv3x3 wgrad, parameter layout") < 2e-3


def test_wgrad_temporal_conv(ops):
    B, Fr, H, W, c = 2, 5, 6, 4, 64
    x = bf(torch.randn(B, Fr, H, W, c, generator=g(1)))
    dy = bf(torch.randn(B, Fr, H, W, c, generator=g(2)))
    w = torch.zeros(c, c, 3, 1, 1, requires_grad=True)
    F.conv3d(x.float().permute(0, 4, 1, 2, 3), w, None, padding=(1, 0, 0)).backward(dy.float().permute(0, 4, 1, 2, 3))
    dW = torch.zeros(c, 3 * c, dtype=torch.float32, device=DEV)
    ops.gemm_wgrad(x.reshape(-1, c).to(DEV), dy.reshape(-1, c).to(DEV), dW, N=c, cin=c, taps=3, mode=2,
                   temporal=(Fr, H * W))
    got = dW.reshape(c, 3, c).permute(0, 2, 1).reshape(c, c, 3, 1, 1)
    assert parity_err(got, w.grad, "temporal wgrad") < 2e-3
    dWt = torch.zeros(c, c, 3, 1, 1, dtype=torch.float32, device=DEV)
    ops.gemm_wgrad(x.reshape(-1, c).to(DEV), dy.reshape(-1, c).to(DEV), dWt, N=c, cin=c, taps=3, mode=2,
                   temporal=(Fr, H * W), torch_layout=True)
    assert parity_err(dWt, w.grad, "temporal wgrad, parameter layout") < 2e-3


@pytest.mark.parametrize("case", [
    dict(M=4100, N=640, K=320),                       # two n tiles, ragged rows (not a multiple of 32), second k tile a quarter full
    dict(M=33333, N=128, K=1280),                     # dY panels past N read zeros; five k tiles; many slabs
    dict(M=2048, N=320, K=64, lda=192, ldy=448),      # row-strided views
    dict(n=4, H=9, W=16, N=320, K=320, taps=9),       # 3x3, rows narrower than a chunk (two image rows per 32)
    dict(n=3, H=24, W=40, N=64, K=128, taps=9),       # 3x3, W not a power of two
    dict(B=2, F=5, S=240, N=320, K=320, taps=3),      # temporal conv
])
def test_wgrad_lds_dma_kernel(ops, case):
    """csrc/wgrad_pp.hip (320 x 256 tile on an LDS-DMA ring; serves mode 0 / stride-1 3x3 / temporal with N, Cin multiples of
    64 and M >= 1024): against fp32 torch on the same 16-bit operands, both weight layouts, fused bias gradient,
    accumulation into a non-zero dW, and the same bits in every run."""
    taps = case.get("taps", 1)
    N, K = case["N"], case["K"]
    kw = dict(N=N, cin=K, taps=taps)
    if taps == 9:
        n, H, W = case["n"], case["H"], case["W"]
        M = n * H * W
        kw.update(mode=1, conv=(H, W, H, W, 1, 0))
    elif taps == 3:
        B, Fr, S = case["B"], case["F"], case["S"]
        M = B * Fr * S
        kw.update(mode=2, temporal=(Fr, S))
    else:
        M = case["M"]
    lda, ldy = case.get("lda", K), case.get("ldy", N)
    A_full = bf(torch.randn(M, lda, generator=g(11))).to(DEV)
    Y_full = bf(torch.randn(M, ldy, generator=g(12))).to(DEV)
    A, dY = A_full[:, :K], Y_full[:, :N]
    a32, y32 = A.float(), dY.float()
    if taps == 9:       # reference: autograd of the fp32 conv on the same operands
        w = torch.zeros(N, K, 3, 3, device=DEV, requires_grad=True)
        F.conv2d(nchw(a32, n, H, W), w, None, padding=1).backward(nchw(y32, n, H, W))
        ref_t = w.grad                                                              # [N, K, 3, 3]
        ref_p = ref_t.permute(0, 2, 3, 1).reshape(N, 9 * K)
    elif taps == 3:
        w = torch.zeros(N, K, 3, 1, 1, device=DEV, requires_grad=True)
        x5 = a32.reshape(B, Fr, S, 1, K).permute(0, 4, 1, 2, 3)
        y5 = y32.reshape(B, Fr, S, 1, N).permute(0, 4, 1, 2, 3)
        F.conv3d(x5, w, None, padding=(1, 0, 0)).backward(y5)
        ref_t = w.grad
        ref_p = ref_t.reshape(N, K, 3).permute(0, 2, 1).reshape(N, 3 * K)
    else:
        ref_p = y32.T @ a32
        ref_t = ref_p
    ref_b = y32.sum(0)

    def run(torch_layout):
        dW = torch.full(ref_t.shape if torch_layout else ref_p.shape, 0.25, dtype=torch.float32, device=DEV)
        db = torch.full((N,), -1.0, dtype=torch.float32, device=DEV)
        ops.gemm_wgrad(A, dY, dW, dbias=db, scale=0.5, torch_layout=torch_layout, **kw)
        return dW, db
    dW, db = run(False)
    assert parity_err(dW - 0.25, 0.5 * ref_p, f"wgrad {case}") < 2e-3
    assert parity_err(db + 1.0, 0.5 * ref_b, "fused bias gradient") < 2e-3
    dWt, dbt = run(True)
    assert parity_err(dWt - 0.25, 0.5 * ref_t, "parameter layout") < 2e-3
    for _ in range(3):
        dW2, db2 = run(False)
        assert torch.equal(dW, dW2) and torch.equal(db, db2)
    assert torch.equal(dbt, db)
    # assign form (torch_layout bit 1): the previous contents are not read
    for tl, ref in ((False, ref_p), (True, ref_t)):
        dWa = torch.full(ref.shape, float("nan"), dtype=torch.float32, device=DEV)
        dba = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
        ops.gemm_wgrad(A, dY, dWa, dbias=dba, scale=0.5, torch_layout=tl, assign=True, **kw)
        assert parity_err(dWa, 0.5 * ref, "assign form") < 2e-3 and parity_err(dba, 0.5 * ref_b, "assign form, bias") < 2e-3


@pytest.mark.parametrize("C,H,W,n,ips", [(320, 9, 16, 6, 1), (320, 9, 16, 6, 3), (64, 16, 16, 4, 2), (128, 72, 64, 2, 1)])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm_backward(ops, C, H, W, n, ips, silu):
    x = bf(torch.randn(n, C, H, W, generator=g(1)) * 1.5 + 0.3)
    dy = bf(torch.randn(n, C, H, W, generator=g(2)))
    gamma = torch.randn(C, generator=g(3), requires_grad=True)
    beta = torch.randn(C, generator=g(4), requires_grad=True)
    xr = x.float().requires_grad_(True)
    if ips == 1:
        y = F.group_norm(xr, 32, gamma, beta, 1e-5)
    else:
        x5 = xr.reshape(n // ips, ips, C, H, W).permute(0, 2, 1, 3, 4)
        y = F.group_norm(x5, 32, gamma, beta, 1e-5).permute(0, 2, 1, 3, 4).reshape(n, C, H, W)
    (F.silu(y) if silu else y).backward(dy.float())
    S = H * W
    xd = rows(x).to(DEV)
    part = torch.empty(ops.groupnorm_scratch_floats(n, S, C, ips), dtype=torch.float32, device=DEV)
    gd, bd = gamma.detach().to(DEV), beta.detach().to(DEV)
    ops.groupnorm(xd, None, n, S, C, ips, gd, bd, 1e-5, silu, torch.empty_like(xd), part)
    dx = torch.empty_like(xd)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.groupnorm_bwd(xd, rows(dy).to(DEV), n, S, C, ips, part, gd, bd, silu, dx, dg, db)
    assert parity_err(nchw(dx.cpu(), n, H, W), xr.grad, "GN dx") < 4e-3
    assert parity_err(dg, gamma.grad, "GN dgamma") < 2e-3 and parity_err(db, beta.grad, "GN dbeta") < 2e-3


@pytest.mark.parametrize("C,with_v", [(64, False), (320, True), (1280, False)])
def test_layernorm_backward(ops, C, with_v):
    from ctrlv_amd.autograd import LayerNormFn
    M, Fr, S = 600, 3, 25
    x = bf(torch.randn(M, C, generator=g(1)) * 1.3 + 0.2)
    dy = bf(torch.randn(M, C, generator=g(2)))
    gamma = torch.randn(C, generator=g(3), requires_grad=True)
    beta = torch.randn(C, generator=g(4), requires_grad=True)
    V = torch.randn(Fr, C, generator=g(5), requires_grad=True) if with_v else None
    xr = x.float().requires_grad_(True)
    xin = xr + V[(torch.arange(M) // S) % Fr] if with_v else xr
    F.layer_norm(xin, (C,), gamma, beta, 1e-5).backward(dy.float())
    xd = x.to(DEV).requires_grad_(True)
    gd, bd = gamma.detach().to(DEV).requires_grad_(True), beta.detach().to(DEV).requires_grad_(True)
    Vd = V.detach().to(DEV).requires_grad_(True) if with_v else None
    y = LayerNormFn.apply(xd, gd, bd, Vd, S, Fr if with_v else 1 << 30)
    y.backward(dy.to(DEV))
    assert parity_err(xd.grad, xr.grad, "LN dx") < 4e-3
    assert parity_err(gd.grad, gamma.grad, "LN dgamma") < 2e-3 and parity_err(bd.grad, beta.grad, "LN dbeta") < 2e-3
    if with_v:
        assert parity_err(Vd.grad, V.grad, "LN dV (frame embedding)") < 4e-3


@pytest.mark.parametrize("C,with_v", [(64, False), (320, True), (320, False), (1280, False)])
def test_norm_backward_adds_the_skip_gradient(ops, C, with_v):
    """skip=True (ctrlv_layernorm_bwd_add / ctrlv_groupnorm_bwd_add): the norm also returns its input for the skip connection
    around the branch; both gradients of x arrive in the norm's backward and its kernel adds the skip's while it writes dx.
    Against torch.autograd on y = norm(x) * a + x * b, and against the unfused form (two autograd outputs summed by torch):
    the fused sum rounds once (fp32 add, one 16-bit rounding) where the unfused rounds dx first."""
    from ctrlv_amd.autograd import GroupNormSiLU, LayerNormFn
    n, S = 4, 150
    M, Fr = n * S, 2
    x = bf(torch.randn(M, C, generator=g(1)) * 1.3 + 0.2)
    w1, w2 = bf(torch.randn(M, C, generator=g(2))), bf(torch.randn(M, C, generator=g(3)))
    gamma = torch.randn(C, generator=g(4))
    beta = torch.randn(C, generator=g(5))
    V = torch.randn(Fr, C, generator=g(6)) if with_v else None
    for kind in ("ln", "gn"):
        if kind == "gn" and with_v:
            continue
        xr = x.float().requires_grad_(True)
        gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        if kind == "ln":
            xin = xr + V[(torch.arange(M) // (S * n // Fr)) % Fr] if with_v else xr
            yr = F.layer_norm(xin, (C,), gr, br, 1e-5)
        else:
            yr = F.silu(F.group_norm(nchw(xr, n, 10, 15), 32, gr, br, 1e-5))
            yr = rows(yr)
        ((yr * w1.float()).sum() + (xr * w2.float()).sum()).backward()
        res = {}
        for fused in (True, False):
            xd = x.to(DEV).requires_grad_(True)
            gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
            Vd = V.to(DEV).requires_grad_(True) if with_v else None
            if kind == "ln":
                args = (xd, gd, bd, Vd, S * n // Fr, Fr if with_v else 1 << 30)
                y, xs = LayerNormFn.apply(*args, True) if fused else (LayerNormFn.apply(*args), xd)
            else:
                args = (xd, gd, bd, n, S, 1, 1e-5, True)
                y, xs = GroupNormSiLU.apply(*args, True) if fused else (GroupNormSiLU.apply(*args), xd)
            torch.autograd.backward([y, xs], [w1.to(DEV), w2.to(DEV)])
            res[fused] = (xd.grad, gd.grad, bd.grad, None if Vd is None else Vd.grad)
            assert parity_err(xd.grad, xr.grad, f"{kind} dx + skip, fused={fused}") < 4e-3
            assert parity_err(gd.grad, gr.grad, "dgamma") < 2e-3 and parity_err(bd.grad, br.grad, "dbeta") < 2e-3
        assert parity_err(res[True][0], res[False][0], "fused vs unfused") < 4e-3
        assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
        if with_v:
            assert torch.equal(res[True][3], res[False][3])
        # only the skip connection carries a gradient: passed through untouched
        xd = x.to(DEV).requires_grad_(True)
        if kind == "ln":
            y, xs = LayerNormFn.apply(xd, gamma.to(DEV), beta.to(DEV), None, 1, 1 << 30, True)
        else:
            y, xs = GroupNormSiLU.apply(xd, gamma.to(DEV), beta.to(DEV), n, S, 1, 1e-5, True, True)
        xs.backward(w2.to(DEV))
        assert torch.equal(xd.grad, w2.to(DEV))


@pytest.mark.parametrize("C", [64, 320])
def test_geglu_feedforward_backward(ops, C):
    """GEGLU projection + output Linear (diffusers FeedForward) through GegluProj / Gemm vs torch.autograd."""
    from ctrlv_amd.autograd import GegluProj, Gemm, GemmSpec
    M = 777
    x = bf(torch.randn(M, C, generator=g(1)))
    w1 = (bf(torch.randn(8 * C, C, generator=g(2)) / math.sqrt(C))).float().requires_grad_(True)
    b1 = bf(torch.randn(8 * C, generator=g(3)) * 0.1).float().requires_grad_(True)
    w2 = (bf(torch.randn(C, 4 * C, generator=g(4)) / math.sqrt(4 * C))).float().requires_grad_(True)
    b2 = bf(torch.randn(C, generator=g(5)) * 0.1).float().requires_grad_(True)
    xr = x.float().requires_grad_(True)
    h, gate = F.linear(xr, w1, b1).chunk(2, dim=-1)
    yr = F.linear(h * F.gelu(gate), w2, b2) + xr
    dy = bf(yr.detach() + 0.5 * torch.randn(M, C, generator=g(6)))
    yr.backward(dy.float())
    xd = x.to(DEV).requires_grad_(True)
    pd = [t.detach().to(DEV).requires_grad_(True) for t in (w1, b1, w2, b2)]
    u = GegluProj.apply(xd, pd[0], pd[1])
    y = Gemm.apply(u, pd[2], pd[3], xd, None, None, GemmSpec())
    assert parity_err(y.detach(), yr.detach(), "FF forward") < 4e-3
    y.backward(dy.to(DEV))
    errs = {"x": rel_l2(xd.grad, xr.grad)}
    for name, a, b in zip(("w1", "b1", "w2", "b2"), pd, (w1, b1, w2, b2)):
        errs[name] = rel_l2(a.grad, b.grad)
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1.5e-2, errs


def _oracle_block(cin, cout, seed):
    import ctrlv_ref as R
    rb = R.seeded_init_(R.SpatioTemporalResBlock(cin, cout, 256, eps=1e-6), seed)
    with torch.no_grad():
        for p in rb.parameters():
            p.copy_(p.to(torch.bfloat16).float())
        rb.time_mixer.mix_factor.fill_(0.25)
    return rb


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128)])
def test_res_block_backward_matches_oracle_autograd(hip_lib, cin, cout):
    """SpatioTemporalResBlock forward + backward through the HIP kernels vs torch.autograd on the oracle block:
    gradients w.r.t. the input, the time embedding, every conv / norm / time_emb_proj parameter and the mix factor."""
    from ctrlv_amd.autograd import res_block_train_forward
    from ctrlv_amd.models.blocks import SpatioTemporalResBlock
    B, Fr, H, W = 2, 3, 8, 8
    rb = _oracle_block(cin, cout, 31)
    x = bf(torch.randn(B * Fr, cin, H, W, generator=g(5))).float()
    temb_b = bf(torch.randn(B, 256, generator=g(6))).float()
    # ---- oracle.  Upstream gradient = d/dy of 0.5 * ||y||^2 plus noise: a pure-noise dY makes the scalar mix_factor
    # gradient (a sum over all outputs) a cancelling random sum whose relative error is unbounded
    xo, to = x.clone().requires_grad_(True), temb_b.clone().requires_grad_(True)
    yo = rb(xo, to.repeat_interleave(Fr, 0), torch.zeros(B, Fr))
    dy = bf(yo.detach() + 0.5 * torch.randn(B * Fr, cout, H, W, generator=g(7))).float()
    yo.backward(dy)
    # ---- HIP: fp32 master parameters on the device, bf16 compute
    blk = SpatioTemporalResBlock(cin, cout, 256, eps=1e-6)
    blk.load_state_dict(rb.state_dict())
    blk.to(DEV)
    for p in blk.parameters():
        p.requires_grad_(True)
    xh = rows(x).to(DEV, torch.bfloat16).requires_grad_(True)
    th = temb_b.to(DEV).requires_grad_(True)
    s, t = blk.spatial_res_block, blk.temporal_res_block
    tabs = [F.linear(F.silu(th), m.time_emb_proj.weight, m.time_emb_proj.bias).contiguous() for m in (s, t)]
    yh = res_block_train_forward(blk, xh, tabs, B, Fr, H, W)
    # the training forward issues the same kernels as the inference path
    e_fwd = parity_err(nchw(yh.detach().float().cpu(), B * Fr, H, W), yo.detach(), "forward")
    assert e_fwd < 6e-3
    yh.backward(rows(dy).to(DEV, torch.bfloat16))
    torch.cuda.synchronize()
    errs = {"x": rel_l2(nchw(xh.grad.float().cpu(), B * Fr, H, W), xo.grad), "temb": rel_l2(th.grad.cpu(), to.grad)}
    ref = dict(rb.named_parameters())
    for name, p in blk.named_parameters():
        assert p.grad is not None, name
        errs[name] = rel_l2(p.grad.float().cpu().reshape(ref[name].shape), ref[name].grad)
    for k, v in errs.items():
        print(f"  {v:.2e}  d/d {k}")
    assert max(errs.values()) < 3e-2, errs


def test_zero_conv_backward(hip_lib):
    """ControlNet zero-conv * conditioning_scale (controlnet.py:331-344): with zero-initialised weights the input gradient is
    exactly zero and the weight gradient is not -- which is how the ControlNet starts to learn."""
    from ctrlv_amd.autograd import zero_conv_train_forward
    C, M = 64, 6 * 64
    conv = torch.nn.Conv2d(C, C, 1).to(DEV)
    torch.nn.init.zeros_(conv.weight); torch.nn.init.zeros_(conv.bias)
    x = bf(torch.randn(M, C, generator=g(1))).to(DEV).requires_grad_(True)
    dy = bf(torch.randn(M, C, generator=g(2))).to(DEV)
    y = zero_conv_train_forward(conv, x, scale=0.8)
    assert float(y.detach().float().abs().max()) == 0.0
    y.backward(dy)
    assert float(x.grad.float().abs().max()) == 0.0
    ref_w = 0.8 * dy.float().T @ x.detach().float()
    assert parity_err(conv.weight.grad.reshape(C, C), ref_w, "zero-conv wgrad") < 2e-3
    assert parity_err(conv.bias.grad, 0.8 * dy.float().sum(0), "zero-conv bias grad") < 2e-3


# ------------------------------------------------------------------------------------------------ attention backward
def _attn_ref(qkv, dout, n_seq, L, C):
    """fp32 autograd of F.scaled_dot_product_attention on the bf16-rounded operands; qkv rows [n_seq*L, 3C]."""
    heads = C // 64
    x = qkv.float().clone().requires_grad_(True)
    f = x.reshape(n_seq, L, 3, heads, 64)
    q, k, v = (f[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    with torch.enable_grad():
        o = F.scaled_dot_product_attention(q, k, v)
        out = o.permute(0, 2, 1, 3).reshape(n_seq * L, C)
        out.backward(dout.float())
    lse = torch.logsumexp((q @ k.transpose(-1, -2)).detach() * 0.125, dim=-1) * math.log2(math.e)     # [n, heads, L]
    return out.detach(), x.grad, lse


@pytest.mark.parametrize("n_img,S,C", [(2, 200, 128), (1, 1100, 64), (3, 64, 320), (1, 2304, 128)])
def test_attention_spatial_backward(ops, n_img, S, C):
    """dq | dk | dv of the spatial core against fp32 autograd; both forward kernels' L (S < 1024: 32 rows per wave,
    S >= 1024: 64), ragged last key / query tiles.  Tolerance: P and dS are rounded to bf16 before their MFMAs and the
    outputs are bf16: parity_err <= 1e-2."""
    qkv = bf(torch.randn(n_img * S, 3 * C, generator=g(1)))
    dout = bf(torch.randn(n_img * S, C, generator=g(2)))
    ref_out, ref_grad, ref_lse = _attn_ref(qkv, dout, n_img, S, C)
    qd, gd = qkv.to(DEV), dout.to(DEV)
    out = torch.empty(n_img * S, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((n_img, C // 64, S), float("nan"), dtype=torch.float32, device=DEV)
    ops.attention_spatial_lse(qd, out, lse, n_img, S, C)
    assert parity_err(out, ref_out, "attention out") < 5e-3
    assert (lse.cpu() - ref_lse).abs().max() < 2e-3
    dqkv = torch.full((n_img * S, 3 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.attention_spatial_bwd(qd, out, gd, lse, dqkv, n_img, S, C)
    for i, name in enumerate(("dq", "dk", "dv")):
        assert parity_err(dqkv[:, i * C:(i + 1) * C], ref_grad[:, i * C:(i + 1) * C], name) < 1e-2
    # deterministic: a second run gives the same bits
    dqkv2 = torch.empty_like(dqkv)
    ops.attention_spatial_bwd(qd, out, gd, lse, dqkv2, n_img, S, C)
    assert torch.equal(dqkv, dqkv2)


def test_attention_spatial_backward_peaked(ops):
    """Large, peaked logits (one key dominates a query; scores of several hundred): P is rebuilt from the saved L.
    With 3x larger queries the bf16 rounding of dS weighs more (measured max-element error 1.3e-2): bound 2e-2."""
    S, C = 320, 64
    qkv = torch.randn(S, 3 * C, generator=g(1))
    qkv[:, :64] *= 3.0
    qkv[300, 64:128] = qkv[7, :64] * 4.0
    qkv = bf(qkv)
    dout = bf(torch.randn(S, C, generator=g(2)))
    ref_out, ref_grad, _ = _attn_ref(qkv, dout, 1, S, C)
    qd, gd = qkv.to(DEV), dout.to(DEV)
    out = torch.empty(S, C, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(1, 1, S, dtype=torch.float32, device=DEV)
    ops.attention_spatial_lse(qd, out, lse, 1, S, C)
    dqkv = torch.empty(S, 3 * C, dtype=torch.bfloat16, device=DEV)
    ops.attention_spatial_bwd(qd, out, gd, lse, dqkv, 1, S, C)
    assert not torch.isnan(dqkv.float()).any()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert parity_err(dqkv[:, i * C:(i + 1) * C], ref_grad[:, i * C:(i + 1) * C], name) < 2e-2


@pytest.mark.parametrize("B,Fr,S,C", [(2, 25, 37, 128), (1, 32, 16, 64), (1, 2, 50, 320), (3, 7, 5, 64)])
def test_attention_temporal_backward(ops, B, Fr, S, C):
    """Temporal core (rows ordered (b, f, s), attention over the frames of each (b, s)): dqkv against fp32 autograd."""
    heads = C // 64
    qkv = bf(torch.randn(B * Fr * S, 3 * C, generator=g(1)))
    dout = bf(torch.randn(B * Fr * S, C, generator=g(2)))
    # (b f s) rows -> sequences (b s) of length f
    perm = qkv.reshape(B, Fr, S, 3 * C).permute(0, 2, 1, 3).reshape(B * S * Fr, 3 * C)
    dperm = dout.reshape(B, Fr, S, C).permute(0, 2, 1, 3).reshape(B * S * Fr, C)
    ref_out, ref_grad, _ = _attn_ref(perm, dperm, B * S, Fr, C)
    ref_out = ref_out.reshape(B, S, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * S, C)
    ref_grad = ref_grad.reshape(B, S, Fr, 3 * C).permute(0, 2, 1, 3).reshape(B * Fr * S, 3 * C)
    qd, gd = qkv.to(DEV), dout.to(DEV)
    out = torch.empty(B * Fr * S, C, dtype=torch.bfloat16, device=DEV)
    ops.attention_temporal(qd, out, B, Fr, S, C)
    assert parity_err(out, ref_out, "temporal out") < 5e-3
    dqkv = torch.full((B * Fr * S, 3 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.attention_temporal_bwd(qd, out, gd, dqkv, B, Fr, S, C)
    assert not torch.isnan(dqkv.float()).any()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert parity_err(dqkv[:, i * C:(i + 1) * C], ref_grad[:, i * C:(i + 1) * C], name) < 1e-2
    assert heads >= 1


# ------------------------------------------------------------------------------------------------ transformer block
@pytest.mark.parametrize("B,order", [(1, "sb"), (2, "sb"), (2, "bs")])
def test_transformer_backward_matches_oracle_autograd(hip_lib, B, order):
    """TransformerSpatioTemporalModel forward + backward through the HIP kernels (GroupNorm, LayerNorm, fused Linears,
    GEGLU, both attention cores, folded cross-attention vectors, frame embedding, folded AlphaBlender) against
    torch.autograd on the oracle: gradients of the input, the CLIP token and EVERY parameter (to_q / to_k / norm2 of the
    one-key cross-attentions: exactly zero on both sides)."""
    import ctrlv_ref as R
    from ctrlv_amd.autograd import transformer_train_forward
    from ctrlv_amd.models.blocks import TransformerSpatioTemporalModel
    Fr, H, W, C, D = 3, 8, 8, 128, 64
    ref = R.seeded_init_(R.TransformerSpatioTemporalModel(C // 64, 64, C, D, time_context_order=order), 17)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.to(torch.bfloat16).float())
        ref.time_mixer.mix_factor.fill_(0.3)
    x = bf(torch.randn(B * Fr, C, H, W, generator=g(5))).float()
    ehs = bf(torch.randn(B, 1, D, generator=g(6))).float()
    xo, eo = x.clone().requires_grad_(True), ehs.clone().requires_grad_(True)
    yo = ref(xo, eo.repeat_interleave(Fr, 0), torch.zeros(B, Fr))
    dy = bf(yo.detach() + 0.5 * torch.randn(B * Fr, C, H, W, generator=g(7))).float()
    yo.backward(dy)

    tr = TransformerSpatioTemporalModel(C // 64, 64, C, D)
    missing = tr.load_state_dict(ref.state_dict(), strict=False)
    assert not missing.missing_keys, missing
    tr.to(DEV)
    for p in tr.parameters():
        p.requires_grad_(True)
    xh = rows(x).to(DEV, torch.bfloat16).requires_grad_(True)
    eh = ehs.reshape(B, D).to(DEV).requires_grad_(True)
    yh = transformer_train_forward(tr, xh, eh, B, Fr, H, W, order)
    assert parity_err(nchw(yh.detach().float().cpu(), B * Fr, H, W), yo.detach(), "forward") < 6e-3
    yh.backward(rows(dy).to(DEV, torch.bfloat16))
    torch.cuda.synchronize()
    errs = {"x": rel_l2(nchw(xh.grad.float().cpu(), B * Fr, H, W), xo.grad),
            "ehs": rel_l2(eh.grad.cpu().reshape(B, 1, D), eo.grad)}
    refp = dict(ref.named_parameters())
    gmax = max(float(q.grad.abs().max()) for q in refp.values() if q.grad is not None)
    zero = []
    for name, p in tr.named_parameters():
        rg = refp[name].grad
        # (softmax over ONE key is the constant 1: the oracle's autograd leaves rounding dust of ~1e-9 there, the HIP
        # path does not compute those projections at all)
        if rg is None or float(rg.abs().max()) <= 1e-6 * gmax:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            zero.append(name)
            continue
        assert p.grad is not None, name
        errs[name] = rel_l2(p.grad.float().cpu().reshape(rg.shape), rg)
    for k, v in errs.items():
        print(f"  {v:.2e}  d/d {k}")
    print("  zero-gradient parameters:", zero)
    assert any("attn2.to_q" in z for z in zero)
    assert max(errs.values()) < 3e-2, errs


@pytest.mark.parametrize("tile", [0, 5, 6])
def test_geglu_projection_raw_output(ops, tile):
    """The training forward's GEGLU GEMM also writes the raw projection (what ctrlv_geglu_bwd consumes): identical bits to
    the plain GEMM on the same packed weight, and u is unchanged by the second output.  Many tiles per workgroup, ragged M."""
    from ctrlv_amd import packing
    M, C = 256 * 300 + 77, 320
    A = bf(torch.randn(M, C, generator=g(1))).to(DEV)
    Wt = torch.randn(8 * C, C, generator=g(2)) / math.sqrt(C)
    b = torch.randn(8 * C, generator=g(3))
    Wp, bp = packing.pack_geglu(Wt, b)
    Wp, bp = Wp.to(DEV), bp.to(DEV)
    u0 = torch.empty(M, 4 * C, dtype=torch.bfloat16, device=DEV)
    ops.gemm(A, Wp, u0, N=8 * C, cin=C, bias=bp, geglu=1, tile=tile)
    raw_ref = torch.empty(M, 8 * C, dtype=torch.bfloat16, device=DEV)
    ops.gemm(A, Wp, raw_ref, N=8 * C, cin=C, bias=bp, tile=tile)
    u1 = torch.full((M, 4 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    raw = torch.full((M, 8 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemm(A, Wp, u1, N=8 * C, cin=C, bias=bp, geglu=1, raw_out=raw, tile=tile)
    assert torch.equal(u0, u1)
    assert torch.equal(raw, raw_ref)


def test_pack_weight_kernel_matches_the_torch_packers(ops):
    """ctrlv_pack_weight (one kernel per trainable weight per step) against packing.py: forward layouts of Linear / 3x3 /
    temporal convs incl. the GEGLU row interleave and row padding to 32, and the role-swapped dgrad layouts (taps
    reversed, channels transposed, N zero-padded to 64)."""
    from ctrlv_amd import packing
    lin = torch.randn(320, 128, generator=g(1)).to(DEV)
    assert torch.equal(ops.pack_weight(lin, 0), packing.pack_linear(lin))
    assert torch.equal(ops.pack_weight(lin, 1), packing.pack_linear(lin.t()))
    odd = torch.randn(40, 128, generator=g(2)).to(DEV)                          # rows padded 40 -> 64, dgrad N 40 -> 64
    assert torch.equal(ops.pack_weight(odd, 0), packing.pack_linear(odd))
    padded = torch.cat([odd, odd.new_zeros(24, 128)], 0)
    assert torch.equal(ops.pack_weight(odd, 1), packing.pack_linear(padded.t()))
    conv = torch.randn(64, 96, 3, 3, generator=g(3)).to(DEV)
    assert torch.equal(ops.pack_weight(conv, 0), packing.pack_conv3x3(conv))
    assert torch.equal(ops.pack_weight(conv, 1), packing.pack_conv3x3(conv.flip(2, 3).transpose(0, 1)))
    tc = torch.randn(64, 64, 3, 1, 1, generator=g(4)).to(DEV).to(torch.bfloat16)
    assert torch.equal(ops.pack_weight(tc, 0), packing.pack_conv_temporal(tc))
    assert torch.equal(ops.pack_weight(tc, 1), packing.pack_conv_temporal(tc.flip(2).transpose(0, 1)))
    gw, gb = torch.randn(512, 64, generator=g(5)).to(DEV), torch.randn(512, generator=g(6)).to(DEV)
    assert torch.equal(ops.pack_weight(gw, 0, geglu=True), packing.pack_geglu(gw, gb)[0])
    assert ops.pack_weight(torch.randn(64, 40, device=DEV), 0) is None             # K = 40: the torch packer pads it
