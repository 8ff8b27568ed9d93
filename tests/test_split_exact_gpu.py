"""Element-exact tests of the SPLIT trunk's lo plane (one e5m2 byte per element, ABI 20) in every kernel that
reads or writes it.

A lo byte is at most half an ulp of its hi element, so a lost, zeroed or misplaced lo byte moves a result by about fp16's
own rounding error -- under the aggregate tolerances of tests/test_trunk_split_gpu.py.  Here the planes are checked element
by element (tests/split_planes.py):
  * exact grids: inputs chosen so that the kernel's fp32 value is exact in any summation order (A on a 2^-3 grid, W on a
    2^-4 grid, power-of-two scales, split operands on a 2^-14 grid, every partial sum a multiple of 2^-15 below 2^8).  Both
    output planes then have exactly one correct answer, compared byte for byte -- MFMA order, split-K slicing and tile
    choice cannot change it;
  * the hardware conversion itself (v_cvt_pk_bf8_f32 / v_cvt_pk_f32_bf8) through axpby_split with a = b = 1;
  * where no exact grid exists (the GEGLU intermediate, the softmax): check_split against an fp64 reference with an
    explicit per-element uncertainty;
  * the norms on inputs whose hi plane is constant per row / group, so that ONLY the lo plane carries the signal.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.parity_utils import parity_err, rel_l2
from tests.split_planes import (EL, LO, assert_planes_equal, check_split, decode_lo, e5m2_bytes, e5m2_rne,
                                expect_split_exact, split)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _pack_in_fp16():
    from ctrlv_amd import packing
    with packing.element_dtype(EL):
        yield


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def lo_plane(*shape):
    """device lo plane pre-filled with the e5m2 NaN byte: a launch must overwrite every element"""
    t = torch.empty(*shape, dtype=LO, device=DEV)
    t.view(torch.uint8).fill_(0x7F)
    return t


def rows_from_nchw(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


# ------------------------------------------------------------------------------------------------ exact grids
def grid(shape, step, lim, seed):
    """uniform values k * step, |k * step| <= lim (float64)"""
    n = int(lim / step)
    return torch.randint(-n, n + 1, shape, generator=g(seed)).double() * step


def split_pair_on_grid(shape, seed, scale=2.0):
    """a split operand (hi fp16, lo e5m2) whose hi + lo is a multiple of 2^-14: hi = an fp16 value >= 2^-4 in magnitude (or
    zero), lo = +-2^e (1 + m / 4) with e in [-12, -9] (or zero) -- every element's lo byte is a different value"""
    hi = (torch.randn(shape, generator=g(seed)) * scale).to(EL)
    hi[hi.abs() < 2.0 ** -4] = 0
    e = torch.randint(-12, -8, shape, generator=g(seed + 1)).double()
    m = torch.randint(0, 4, shape, generator=g(seed + 2)).double()
    s = torch.randint(0, 2, shape, generator=g(seed + 3)).double() * 2 - 1
    lo = s * torch.exp2(e) * (1 + m / 4)
    lo[torch.rand(shape, generator=g(seed + 4)) < 0.05] = 0
    lo = lo.to(LO)
    return hi, lo, hi.double() + lo.double()


def assert_exact_grid(acc_abs, v, terms):
    """The precondition of a bit-exact comparison, on the host: every MFMA partial sum is a multiple of 2^-7 below 2^17
    (acc_abs = sum |a w| per element), every epilogue term a multiple of 2^-15, and any partial sum of the epilogue below 2^8."""
    assert float(acc_abs.max()) < 2.0 ** 16
    tot = torch.zeros_like(v)
    for t in terms:
        t = torch.as_tensor(t, dtype=torch.float64).expand_as(v)
        assert torch.equal(torch.round(t * 2.0 ** 15), t * 2.0 ** 15), "epilogue term off the 2^-15 grid"
        tot = tot + t.abs()
    assert float(tot.max()) < 2.0 ** 8
    assert torch.equal(v.float().double(), v)


def test_lo_decode_every_byte(ops):
    """Hardware decode (v_cvt_pk_f32_bf8): x = +-0, x_lo = every byte, r = +-0 -> the hi plane IS the decoded byte (e5m2 is
    the top byte of fp16), bit for bit; the inf bytes give inf, the NaN bytes NaN."""
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    z = torch.where(b >= 128, torch.tensor(-0.0), torch.tensor(0.0)).to(EL)       # -0 + -v keeps the sign of a zero byte
    yh, yl = torch.empty(256, dtype=EL, device=DEV), lo_plane(256)
    ops.axpby_split(z.to(DEV), b.view(LO).to(DEV), z.to(DEV), 1.0, 1.0, yh, yl)
    got = yh.cpu().view(torch.int16).to(torch.int32) & 0xFFFF
    exp = b.to(torch.int32) << 8
    exp16 = exp.to(torch.int16).view(EL)
    nan = torch.isnan(exp16)
    assert int(nan.sum()) == 6 and int(torch.isinf(exp16).sum()) == 2
    bad = (got != exp) & ~nan
    assert not bad.any(), [(hex(int(i)), hex(int(got[i]))) for i in torch.nonzero(bad)[:8, 0]]
    assert torch.isnan(yh.cpu()[nan]).all()
    fin = torch.isfinite(exp16)
    assert (yl.cpu().view(torch.uint8)[fin] & 0x7F == 0).all()       # an exact value: a zero residual


def _encode_grid():
    """v = H + d, exact in fp32: H an fp16 value of every exponent -14..14 (ulp 2^-24 .. 2^4), d an fp16 value up to one
    ulp of H -- so v - rne16(v) covers every e5m2 binade, the subnormals (|v| around 2^-4 .. 2^-1), exact ties between two
    e5m2 values, [2^-17, 2^-16), zero and both signs."""
    gen = g(11)
    H, D = [], []
    for eh in range(-14, 15):
        ulp = 2.0 ** (eh - 10)
        n = 4096
        h = torch.exp2(torch.full((n,), float(eh), dtype=torch.float64)) * (1 + torch.randint(0, 1024, (n,), generator=gen).double() / 1024)
        # residuals: random fp16 values within +-ulp (some round hi to the neighbour: residual crosses zero)
        d = (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * ulp
        d = d.to(EL).double()
        # exact e5m2 ties and their neighbours at every binade below ulp / 2
        k = torch.arange(-17, max(-17, eh - 10), dtype=torch.float64)
        ties = torch.cat([torch.exp2(k) * (1 + (2 * j + 1) / 8) for j in range(4)] + [torch.exp2(k)])
        ties = torch.cat([ties, -ties, torch.tensor([2.0 ** -17, 1.5 * 2.0 ** -17, 1.25 * 2.0 ** -17, -2.0 ** -17,
                                                     -1.75 * 2.0 ** -17, 0.0, -0.0], dtype=torch.float64)])
        ties = ties[ties.abs() < ulp / 2]
        d[:ties.numel()] = ties.to(EL).double()
        H.append(h.to(EL).double())
        D.append(d)
    H, D = torch.cat(H), torch.cat(D)
    H, D = torch.cat([H, -H]), torch.cat([D, -D])
    keep = (H + D).float().double() == H + D          # v exact in fp32 (a large H and a tiny d span more than 24 bits)
    H, D = H[keep], D[keep]
    n8 = H.numel() // 8 * 8
    return H[:n8], D[:n8]


def test_lo_encode_grid(ops):
    """Hardware encode (v_cvt_pk_bf8_f32) against the host model (tests/split_planes.py e5m2_rne: round to nearest even,
    subnormals down to 2^-16), byte for byte, through axpby_split: (y, y_lo) = split(x + x_lo + r) with x + r exact."""
    H, D = _encode_grid()
    v = H + D
    assert torch.equal(v.float().double(), v)
    hi_e, lo_e = expect_split_exact(v)
    res = v - hi_e.double()
    assert (res.abs() < 2.0 ** -16).sum() > 500 and ((res.abs() >= 2.0 ** -17) & (res.abs() < 2.0 ** -16)).sum() > 50
    assert (e5m2_rne(res) == 0).sum() > 100 and (res < 0).sum() > 1000
    xl = torch.zeros(H.numel(), dtype=torch.uint8).view(LO)
    yh, yl = torch.empty(H.numel(), dtype=EL, device=DEV), lo_plane(H.numel())
    ops.axpby_split(H.to(EL).to(DEV), xl.to(DEV), D.to(EL).to(DEV), 1.0, 1.0, yh, yl)
    got_l = yl.cpu().view(torch.uint8)
    bad = got_l != lo_e
    if bad.any():
        i = torch.nonzero(bad)[:6, 0]
        raise AssertionError(f"{int(bad.sum())} lo bytes differ from round-to-nearest-even: residuals {res[i].tolist()} "
                             f"expected {[hex(int(x)) for x in lo_e[i]]} got {[hex(int(x)) for x in got_l[i]]}")
    assert_planes_equal(yh, yl, hi_e, lo_e, "axpby_split encode")
    # and with a lo operand: x_lo = those bytes, r = 0 -> split(fp32(hi + lo)) (the decode, the fp32 sum, the encode; hi + lo
    # is not v itself: a residual rounded up to half an ulp makes a tie, and a wide pair rounds in fp32)
    yh2, yl2 = torch.empty_like(yh), lo_plane(H.numel())
    ops.axpby_split(hi_e.to(DEV), lo_e.view(LO).to(DEV), torch.zeros_like(yh), 1.0, 1.0, yh2, yl2)
    h2, l2 = expect_split_exact((hi_e.float() + decode_lo(lo_e).float()).double())
    assert_planes_equal(yh2, yl2, h2, l2, "axpby_split round trip")


def _mode0_case(epi, M, N, K=256):
    from ctrlv_amd import packing
    A = grid((M, K), 2.0 ** -3, 1.0, 1)
    W = grid((N, K), 2.0 ** -4, 0.5, 2)
    bias = grid((N,), 2.0 ** -3, 4.0, 3)
    V = grid((7, N), 2.0 ** -3, 2.0, 6)
    r1h, r1l, r1 = split_pair_on_grid((M, N), 10)
    r2h, r2l, r2 = split_pair_on_grid((M, N), 20)
    acc = A @ W.T
    kw = dict(N=N, cin=K, bias=bias.float().to(DEV))
    Ad = A.to(EL).to(DEV)
    vidx = (torch.arange(M) // 13) % 7
    if epi == "bias":
        terms = [acc, bias]
    elif epi == "r1":
        kw.update(R1=r1h.to(DEV), R1_lo=r1l.to(DEV), s1=0.5, s_acc=0.5)
        terms = [0.5 * acc, 0.5 * bias, 0.5 * r1]
    elif epi == "r1v":
        kw.update(R1=r1h.to(DEV), R1_lo=r1l.to(DEV), V=V.float().to(DEV), vmode=1, vdiv=13, vmod=7)
        terms = [acc, bias, r1, V[vidx]]
    elif epi == "r1r2":
        kw.update(R1=r1h.to(DEV), R1_lo=r1l.to(DEV), s1=0.5, R2=r2h.to(DEV), R2_lo=r2l.to(DEV), s2=-0.5, s_acc=0.5)
        terms = [0.5 * acc, 0.5 * bias, 0.5 * r1, -0.5 * r2]
    else:       # bias_a2: the skip-concat shortcut, A | A2 split on K
        kw.update(A2=Ad[:, 128:].contiguous(), c_split=128)
        Ad = Ad[:, :128].contiguous()
        terms = [acc, bias]
    v = sum(torch.as_tensor(t).expand(M, N) for t in terms)
    assert_exact_grid(A.abs() @ W.abs().T, v, terms)
    return Ad, packing.pack_linear(W.float()).to(DEV), kw, v


@pytest.mark.parametrize("N", [320, 640, 1280])
@pytest.mark.parametrize("M", [300, 2048 + 77])
@pytest.mark.parametrize("epi", ["bias", "r1", "r1v", "r1r2", "bias_a2"])
def test_gemm_split_exact_mode0(ops, epi, M, N):
    """mode 0 with every trunk epilogue: both planes byte for byte against the exact expectation -- the 2-stage kernel
    (M = 300) and the ping-pong tiles (M = 2125: a 77-row M tail, M % 32 = 13) alike."""
    Ad, Wd, kw, v = _mode0_case(epi, M, N)
    hi_e, lo_e = expect_split_exact(v)
    for tile in ([0, 1] if M > 1024 else [0]):
        hi = torch.full((M, N), float("nan"), dtype=EL, device=DEV)
        lo = lo_plane(M, N)
        ops.gemm(Ad, Wd, hi, out_lo=lo, tile=tile, **kw)
        assert_planes_equal(hi, lo, hi_e, lo_e, f"{epi} M {M} N {N} tile {tile}")


def _conv_case(kind, H, W, n, cin, cout, wlim=0.5):
    """(x rows, packed weights, gemm keywords, exact value) of a trunk conv writer on the exact grid"""
    from ctrlv_amd import packing
    x = grid((n, cin, H, W), 2.0 ** -3, 1.0, 1)
    b = grid((cout,), 2.0 ** -3, 4.0, 3)
    if kind.startswith("conv"):
        wt = grid((cout, cin, 3, 3), 2.0 ** -4, wlim, 2)
        wd = packing.pack_conv3x3(wt.float()).to(DEV)
        if kind == "conv_s2":
            Ho, Wo, stride, up = H // 2, W // 2, 2, 0
            acc = F.conv2d(x, wt, None, stride=2, padding=1)
            acc_abs = F.conv2d(x.abs(), wt.abs(), None, stride=2, padding=1)
        elif kind == "conv_up":
            Ho, Wo, stride, up = 2 * H, 2 * W, 1, 1
            xu = F.interpolate(x, scale_factor=2.0, mode="nearest")
            acc, acc_abs = F.conv2d(xu, wt, None, padding=1), F.conv2d(xu.abs(), wt.abs(), None, padding=1)
        else:
            Ho, Wo, stride, up = H, W, 1, 0
            acc, acc_abs = F.conv2d(x, wt, None, padding=1), F.conv2d(x.abs(), wt.abs(), None, padding=1)
        kw = dict(N=cout, cin=cin, taps=9, mode=1, conv=(H, W, Ho, Wo, stride, up), bias=b.float().to(DEV))
    else:
        Ho, Wo, Fr = H, W, 3 if n % 3 == 0 else 2
        wt = grid((cout, cin, 3, 1, 1), 2.0 ** -4, wlim, 2)
        wd = packing.pack_conv_temporal(wt.float()).to(DEV)

        def c3(xx, ww):
            x5 = xx.reshape(n // Fr, Fr, cin, H, W).permute(0, 2, 1, 3, 4)
            return F.conv3d(x5, ww, None, padding=(1, 0, 0)).permute(0, 2, 1, 3, 4).reshape(n, cout, H, W)
        acc, acc_abs = c3(x, wt), c3(x.abs(), wt.abs())
        kw = dict(N=cout, cin=cin, taps=3, mode=2, temporal=(Fr, H * W), bias=b.float().to(DEV))
    acc, acc_abs = rows_from_nchw(acc), rows_from_nchw(acc_abs)
    M = n * Ho * Wo
    terms = [acc, b]
    if kind.endswith("_r1"):
        r1h, r1l, r1 = split_pair_on_grid((M, cout), 10)
        kw.update(R1=r1h.to(DEV), R1_lo=r1l.to(DEV), s_acc=0.5)
        terms = [0.5 * acc, 0.5 * b, r1]
    v = sum(torch.as_tensor(t).expand(M, cout) for t in terms)
    assert_exact_grid(acc_abs, v, terms)
    return rows_from_nchw(x).to(EL).to(DEV), wd, kw, v


# gns: whether the launcher serves GroupNorm partials for the launch (the {R1} writers with whole 64-row wave tiles per
# image: S % 64 == 0 -- csrc/gemm_pp_m0.hip ctrlv_gemm_gn_partials_serves)
@pytest.mark.parametrize("kind,H,W,n,cin,cout,gns", [
    ("conv_r1", 8, 32, 6, 64, 320, True), ("conv_r1", 9, 16, 9, 64, 640, False), ("conv_s2", 16, 32, 9, 64, 320, False),
    ("conv_up", 8, 16, 5, 64, 320, False), ("temporal_r1", 8, 16, 9, 64, 320, True), ("temporal_r1", 8, 8, 6, 64, 1280, True)])
def test_gemm_split_exact_convs(ops, kind, H, W, n, cin, cout, gns):
    """modes 1 and 2 (row-halo conv3x3, stride 2, nearest-up, temporal conv): both planes byte for byte, every tile; the
    GroupNorm-partials launches (GNS + LO) of the cases the launcher serves."""
    xd, wd, kw, v = _conv_case(kind, H, W, n, cin, cout)
    M = v.shape[0]
    hi_e, lo_e = expect_split_exact(v)
    for tile in ([0, 1] if M >= 1024 else [0]):
        hi = torch.full((M, cout), float("nan"), dtype=EL, device=DEV)
        lo = lo_plane(M, cout)
        ops.gemm(xd, wd, hi, out_lo=lo, tile=tile, **kw)
        assert_planes_equal(hi, lo, hi_e, lo_e, f"{kind} {H}x{W} n {n} cout {cout} tile {tile}")
    assert ops.gemm_gn_partials_serves(xd, wd, hi, out_lo=lo, **kw) == gns
    if gns:
        ips = kw["temporal"][0] if kw["mode"] == 2 else 1
        part = torch.full((ops.groupnorm_fused_scratch_floats(n, H * W, ips),), float("nan"), dtype=torch.float32, device=DEV)
        hi = torch.full((M, cout), float("nan"), dtype=EL, device=DEV)
        lo = lo_plane(M, cout)
        ops.gemm(xd, wd, hi, out_lo=lo, gn_partials=part, **kw)
        assert_planes_equal(hi, lo, hi_e, lo_e, f"{kind} with GroupNorm partials")


@pytest.mark.parametrize("kind,H,W,n,cin", [("conv_r1", 5, 8, 6, 1280), ("temporal_r1", 5, 8, 4, 2560)])
def test_gemm_split_exact_splitk(ops, kind, H, W, n, cin):
    """The lo path of the split-K reduce (csrc/gemm.hip splitk_reduce_kernel: R1_lo, out_lo): the split launch, the unsplit
    launch and the exact expectation agree byte for byte in both planes."""
    xd, wd, kw, v = _conv_case(kind, H, W, n, cin, 1280, wlim=0.25)
    M = v.shape[0]
    hi_e, lo_e = expect_split_exact(v)
    hi = torch.full((M, 1280), float("nan"), dtype=EL, device=DEV)
    lo = lo_plane(M, 1280)
    assert ops.gemm_splitk_slices(xd, wd, hi, out_lo=lo, **kw) >= 2
    ops.gemm(xd, wd, hi, out_lo=lo, **kw)
    assert_planes_equal(hi, lo, hi_e, lo_e, f"{kind} split-K")
    hi1, lo1 = torch.full_like(hi, float("nan")), lo_plane(M, 1280)
    ops.gemm(xd, wd, hi1, out_lo=lo1, splitk=False, **kw)
    assert_planes_equal(hi1, lo1, hi_e, lo_e, f"{kind} unsplit")


@pytest.mark.parametrize("M,epi", [(1000, "r1"), (2048 + 72, "r1r2"), (256 * 9, "r1v")])
def test_ff_fused_split_per_element(ops, M, epi):
    """The fused C = 320 feed-forward with split R1 / R2 / out, per element: v64 = the second projection in fp64 over the
    u the separate GEGLU launch writes (the same arithmetic: tests/test_trunk_split_gpu.py test_ff_fused_split), err64 =
    the worst-case fp32 summation bound over K = 1280 from |u| |W2|.  The trunk operand sits near 96 (ulp 2^-4) so that
    the bound stays far under an ulp / 16 and the lo plane is visible."""
    from ctrlv_amd import packing
    C = 320
    x = torch.randn(M, C, generator=g(1)).to(EL)
    W1 = torch.randn(8 * C, C, generator=g(2)) / math.sqrt(C)
    b1 = torch.randn(8 * C, generator=g(3)) * 0.1
    W2 = torch.randn(C, 4 * C, generator=g(4)) / math.sqrt(4 * C)
    b2 = torch.randn(C, generator=g(5)) * 0.1
    W1p, b1p = packing.pack_geglu(W1, b1)
    W2p = packing.pack_linear(W2)
    r1h, r1l = split(torch.randn(M, C, generator=g(6)) * 4 + 96)
    r2h, r2l = split(torch.randn(M, C, generator=g(7)) * 4 + 96)
    V = torch.randn(9, C, generator=g(8))
    kw = dict(R1=r1h.to(DEV), R1_lo=r1l.to(DEV))
    s_acc, s1, s2 = 1.0, 1.0, 0.0
    if epi == "r1r2":
        kw.update(R2=r2h.to(DEV), R2_lo=r2l.to(DEV), s_acc=0.5, s1=0.5, s2=0.5)
        s_acc, s1, s2 = 0.5, 0.5, 0.5
    if epi == "r1v":
        kw.update(V=V.to(DEV), vmode=1, vdiv=256, vmod=9)
    xd, W1d, b1d, W2d, b2d = x.to(DEV), W1p.to(DEV), b1p.to(DEV), W2p.to(DEV), b2.to(DEV)
    w1f, w2f = ops.ff_fused_pack(W1d, b1d, W2d)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    ops.ff_fused(xd, w1f, w2f, hi, bias=b2d, out_lo=lo, **kw)
    u = torch.empty(M, 4 * C, dtype=EL, device=DEV)
    ops.gemm(xd, W1d, u, N=8 * C, cin=C, bias=b1d, geglu=1)
    u64, w2 = u.cpu().double(), W2p[:C].double()
    proj = u64 @ w2.T + b2.double()
    err = s_acc * (4 * C + 8) * 2.0 ** -24 * (u64.abs() @ w2.abs().T + b2.double().abs())
    v = s_acc * proj + s1 * (r1h.double() + decode_lo(r1l))
    if epi == "r1r2":
        v = v + s2 * (r2h.double() + decode_lo(r2l))
    if epi == "r1v":
        v = v + V.double()[(torch.arange(M) // 256) % 9]
    err = err + v.abs() * 2.0 ** -22           # (the epilogue's own few fp32 roundings)
    check_split(hi, lo, v, err, f"ff_fused {epi} M {M}")


# ------------------------------------------------------------------------------------------------ norms, lo-only signal
def lo_only_rows(M, C, level, seed):
    """split rows whose hi plane is ONE value per row (around `level`) and whose lo plane carries a different value in every
    column: +-2^e (1 + m / 4) with e in the top four binades under half an ulp of hi"""
    gen = g(seed)
    hi_row = (level * (1 + 0.01 * torch.randn(M, 1, generator=gen))).to(EL)
    hi = hi_row.expand(M, C).contiguous()
    emax = int(math.floor(math.log2(level))) - 11
    e = torch.randint(emax - 3, emax + 1, (M, C), generator=gen).double()
    m = torch.randint(0, 4, (M, C), generator=gen).double()
    s = torch.randint(0, 2, (M, C), generator=gen).double() * 2 - 1
    lo = (s * torch.exp2(e) * (1 + m / 4)).to(LO)
    return hi, lo, hi.double() + lo.double()


# (|hi| around 1000: the fp32 mean of the row carries its own rounding, ~1e-3 of the lo plane's spread)
LO_ONLY_TOL = {1.0: 3e-3, 1000.0: 1e-2}


@pytest.mark.parametrize("level", [1.0, 1000.0])
@pytest.mark.parametrize("C", [320, 640, 1280])
def test_layernorm_lo_only_input(ops, C, level):
    """LayerNorm of rows whose signal is in the lo plane only: LN(hi) would collapse to beta; ignoring x_lo, reading it from
    the wrong column or a variance with cancellation shows as an O(1) error against fp64."""
    M = 600
    hi, lo, x = lo_only_rows(M, C, level, 1)
    gamma, beta = torch.randn(C, generator=g(2)), torch.randn(C, generator=g(3)) * 0.1
    y = torch.full((M, C), float("nan"), dtype=EL, device=DEV)
    ops.layernorm(hi.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-5, y, x_lo=lo.to(DEV))
    ref = F.layer_norm(x, (C,), gamma.double(), beta.double(), 1e-5)
    assert parity_err(y, ref.float(), f"LN lo-only C {C} level {level}") < LO_ONLY_TOL[level]


def _gn_ref(xs, n, C, H, W, ips, gamma, beta, eps):
    xs = xs.reshape(n, H, W, C).permute(0, 3, 1, 2)
    if ips == 1:
        r = F.group_norm(xs, 32, gamma.double(), beta.double(), eps)
    else:
        x5 = xs.reshape(n // ips, ips, C, H, W).permute(0, 2, 1, 3, 4)
        r = F.group_norm(x5, 32, gamma.double(), beta.double(), eps).permute(0, 2, 1, 3, 4).reshape(n, C, H, W)
    return rows_from_nchw(F.silu(r).float())


def lo_only_groups(n, S, C, ips, level, seed):
    """split rows [n * S, C] whose hi plane is one value per (stat image, group) and whose lo plane differs everywhere"""
    gen = g(seed)
    hi_g = (level * (1 + 0.01 * torch.randn(n // ips, 1, 32, 1, generator=gen))).to(EL)
    hi = hi_g.expand(n // ips, ips * S, 32, C // 32).reshape(n * S, C).contiguous()
    _, lo, _ = lo_only_rows(n * S, C, level, seed + 1)
    return hi, lo, hi.double() + lo.double()


@pytest.mark.parametrize("level", [1.0, 1000.0])
@pytest.mark.parametrize("C,H,W,n,ips", [(320, 9, 16, 6, 1), (320, 9, 16, 6, 3), (640, 8, 8, 4, 2)])
def test_groupnorm_lo_only_input(ops, C, H, W, n, ips, level):
    """GroupNorm(+SiLU) with the signal in the lo plane only: plain, and as the skip concat with the lo plane on each half."""
    S = H * W
    hi, lo, x = lo_only_groups(n, S, C, ips, level, 1)
    gamma, beta = torch.randn(C, generator=g(2)), torch.randn(C, generator=g(3)) * 0.1
    ref = _gn_ref(x, n, C, H, W, ips, gamma, beta, 1e-5)
    part = torch.empty(ops.groupnorm_scratch_floats(n, S, C, ips), dtype=torch.float32, device=DEV)
    y = torch.full((n * S, C), float("nan"), dtype=EL, device=DEV)
    ops.groupnorm(hi.to(DEV), None, n, S, C, ips, gamma.to(DEV), beta.to(DEV), 1e-5, True, y, part, x_lo=lo.to(DEV))
    assert parity_err(y, ref, f"GN lo-only C {C} ips {ips} level {level}") < LO_ONLY_TOL[level]
    c1 = C // 2
    y2 = torch.full_like(y, float("nan"))
    ops.groupnorm(hi[:, :c1].contiguous().to(DEV), hi[:, c1:].contiguous().to(DEV), n, S, C, ips, gamma.to(DEV), beta.to(DEV),
                  1e-5, True, y2, part, x_lo=lo[:, :c1].contiguous().to(DEV), x2_lo=lo[:, c1:].contiguous().to(DEV))
    assert parity_err(y2, ref, "GN lo-only, concat") < LO_ONLY_TOL[level]


@pytest.mark.parametrize("level", [1.0, 1000.0])
def test_groupnorm_from_partials_lo_only_input(ops, level):
    """The GNS + LO writer with W = 0 and bias = 0 writes out = R1 exactly (both planes) and the chunk partials of hi + lo;
    GroupNorm from those partials on an input whose signal is in the lo plane only."""
    from ctrlv_amd import packing
    H, W, n, cin, C = 8, 32, 6, 64, 320
    S, M = H * W, n * H * W
    hi_in, lo_in, x = lo_only_groups(n, S, C, 1, level, 5)
    hi_e, lo_e = expect_split_exact(x)
    xd = torch.randn(M, cin, generator=g(1)).to(EL).to(DEV)
    wd = packing.pack_conv3x3(torch.zeros(C, cin, 3, 3)).to(DEV)
    kw = dict(N=C, cin=cin, taps=9, mode=1, conv=(H, W, H, W, 1, 0), bias=torch.zeros(C, device=DEV),
              R1=hi_in.to(DEV), R1_lo=lo_in.to(DEV), s_acc=0.5)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    assert ops.gemm_gn_partials_serves(xd, wd, hi, out_lo=lo, **kw)
    part = torch.full((ops.groupnorm_fused_scratch_floats(n, S, 1),), float("nan"), dtype=torch.float32, device=DEV)
    ops.gemm(xd, wd, hi, out_lo=lo, gn_partials=part, **kw)
    assert_planes_equal(hi, lo, hi_e, lo_e, "R1 through the GNS + LO epilogue")
    gamma, beta = torch.randn(C, generator=g(6)), torch.randn(C, generator=g(7)) * 0.1
    y = torch.full((M, C), float("nan"), dtype=EL, device=DEV)
    ops.groupnorm_from_partials(hi, n, S, C, 1, gamma.to(DEV), beta.to(DEV), 1e-6, True, y, part, x_lo=lo)
    assert parity_err(y, _gn_ref(x, n, C, H, W, 1, gamma, beta, 1e-6), f"GN from partials, lo-only, {level}") < LO_ONLY_TOL[level]


# ------------------------------------------------------------------------------------------------ temporal_fused, LO
def _tf_weights(ops, C=320, wo_scale=1.0, seed=3):
    from ctrlv_amd import packing
    wq, wk, wv = (torch.randn(C, C, generator=g(seed + i)) / math.sqrt(C) for i in range(3))
    wo = torch.randn(C, C, generator=g(seed + 4)) / math.sqrt(C) * wo_scale
    wqkv = packing.pack_qkv(wq, wk, wv).to(DEV)
    wop = packing.pack_linear(wo).to(DEV)
    return (wq, wk, wv, wo), wqkv, wop, ops.temporal_fused_pack(wqkv, wop)


def _vkw(vm, vt, B, Fr, S):
    if not vm:
        return {}
    if vm == 1:
        return dict(V=vt.float().to(DEV), vmode=1, vdiv=Fr * S)
    return dict(V=vt.float().to(DEV), vmode=2, vdiv=Fr * S, vS=S, vmod=B)


def _vrows(vm, vt, B, Fr, S):
    M = B * Fr * S
    m = torch.arange(M)
    idx = (m // (Fr * S)) if vm == 1 else ((m // (Fr * S)) * S + m % S) % B
    return vt.double()[idx]


TF_CASES = [(1, 3, 37, 1), (2, 14, 19, 2), (2, 25, 13, 1), (1, 32, 11, 2), (2, 25, 72, 2)]


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("B,Fr,S,vm", TF_CASES)
def test_temporal_fused_lo_residual_exact(ops, B, Fr, S, vm, ln):
    """The LO instantiation with W_out = 0: out = R1 + bias + V, exact -- both planes byte for byte.  Pins where every lo
    byte of R1 is read and where every byte of out_lo is written (partial pixel groups, F up to 32, both row-vector modes,
    with and without the LayerNorm prologue)."""
    C, M = 320, B * Fr * S
    _, _, _, wf = _tf_weights(ops, wo_scale=0.0)
    r1h, r1l, r1 = split_pair_on_grid((M, C), 30)
    bias = grid((C,), 2.0 ** -3, 4.0, 31)
    vt = grid((B, C), 2.0 ** -3, 2.0, 32)
    v = r1 + bias
    if vm:
        v = v + _vrows(vm, vt, B, Fr, S)
    assert_exact_grid(torch.zeros(1), v, [r1, bias] + ([_vrows(vm, vt, B, Fr, S)] if vm else []))
    hi_e, lo_e = expect_split_exact(v)
    r1d = r1h.to(DEV)
    kw = dict(bias=bias.float().to(DEV), R1=r1d, R1_lo=r1l.to(DEV), **_vkw(vm, vt, B, Fr, S))
    if ln:      # (the block's layout: the normalised rows are the residual's)
        kw["ln"] = (torch.randn(C, generator=g(33)).to(DEV), torch.randn(C, generator=g(34)).to(DEV), 1e-5)
    x = r1d if ln else torch.randn(M, C, generator=g(35)).to(EL).to(DEV)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    assert ops.temporal_fused_serves(x, wf, hi, B, Fr, S, out_lo=lo, **kw)
    ops.temporal_fused(x, wf, hi, B, Fr, S, out_lo=lo, **kw)
    assert_planes_equal(hi, lo, hi_e, lo_e, f"temporal_fused LO B{B} F{Fr} S{S} vm{vm} ln{ln}")


def _tf_reference(x, ws, bias, r1, B, Fr, S, vrows=None, ln=None):
    """fp64 reference of the block at the launches' rounding points: (LN output,) q, k, v and the attention output rounded
    to fp16; returns (v64, err64) -- err64 covers one fp16 ulp of every attention output element (the kernel's softmax
    rounds differently) and the fp32 sums."""
    C, heads, M = 320, 5, B * Fr * S
    wq, wk, wv, wo = (w.to(EL).double() for w in ws)
    if ln is not None:
        x = F.layer_norm(x, (C,), ln[0].double(), ln[1].double(), ln[2]).to(EL).double()
    q, k, v = ((x @ w.T).to(EL).double() for w in (wq, wk, wv))

    def tok(t):
        return t.reshape(B, Fr, S, heads, 64).permute(0, 2, 3, 1, 4).reshape(B * S, heads, Fr, 64)
    att = F.scaled_dot_product_attention(tok(q), tok(k), tok(v))
    att = att.reshape(B, S, heads, Fr, 64).permute(0, 3, 1, 2, 4).reshape(M, C)
    a16 = att.to(EL).double()
    out = a16 @ wo.T + bias.double() + r1
    if vrows is not None:
        out = out + vrows
    # (an attention output element may differ by about an fp16 ulp of the row's scale: 2^-9 (|a| + rms(a)))
    ea = 2.0 ** -9 * (a16.abs() + a16.pow(2).mean(1, keepdim=True).sqrt())
    err = ea @ wo.abs().T + (C + 8) * 2.0 ** -24 * (a16.abs() @ wo.abs().T) + out.abs() * 2.0 ** -22
    return out, err


@pytest.mark.parametrize("B,Fr,S,vm", TF_CASES[:4])
def test_temporal_fused_lo_branch(ops, B, Fr, S, vm):
    """The LO instantiation with a real branch: with R1_lo = 0 the hi plane equals the plain instantiation's output bit for
    bit; then the lo plane per element (check_split) against fp64 at the launches' rounding points.  R1 sits near 96 and the
    branch is small, so the reference's uncertainty stays under an ulp / 16 of hi."""
    C, M = 320, B * Fr * S
    ws, _, _, wf = _tf_weights(ops, wo_scale=0.05)
    x = torch.randn(M, C, generator=g(40)).to(EL)
    r1h, r1l = split(torch.randn(M, C, generator=g(41)) * 4 + 96)
    bias = torch.randn(C, generator=g(42)) * 0.1
    vt = torch.randn(B, C, generator=g(43)) * 0.1
    vkw = _vkw(vm, vt, B, Fr, S)
    xd = x.to(DEV)
    plain = torch.full((M, C), float("nan"), dtype=EL, device=DEV)
    ops.temporal_fused(xd, wf, plain, B, Fr, S, bias=bias.to(DEV), R1=r1h.to(DEV), **vkw)
    zl = torch.zeros(M, C, dtype=torch.uint8).view(LO).to(DEV)
    hi0, lo0 = torch.full_like(plain, float("nan")), lo_plane(M, C)
    ops.temporal_fused(xd, wf, hi0, B, Fr, S, bias=bias.to(DEV), R1=r1h.to(DEV), R1_lo=zl, out_lo=lo0, **vkw)
    assert torch.equal(hi0, plain)
    hi, lo = torch.full_like(plain, float("nan")), lo_plane(M, C)
    ops.temporal_fused(xd, wf, hi, B, Fr, S, bias=bias.to(DEV), R1=r1h.to(DEV), R1_lo=r1l.to(DEV), out_lo=lo, **vkw)
    vr = _vrows(vm, vt.float(), B, Fr, S) if vm else None
    v0, err = _tf_reference(x.double(), ws, bias, r1h.double(), B, Fr, S, vr)
    check_split(hi0, lo0, v0, err, f"temporal_fused LO branch, R1_lo = 0, B{B} F{Fr} S{S}")
    v1 = v0 + decode_lo(r1l)
    check_split(hi, lo, v1, err, f"temporal_fused LO branch B{B} F{Fr} S{S}")


def _fallback(ops, g0h, g0l, wqkv, wop, ln, bias, B, Fr, S, vkw):
    """the four launches the fused block replaces, split mode (csrc/plan.hip / models/blocks.py fallback): LayerNorm of the
    hi plane, q|k|v, attention, out-projection with the split residual"""
    M, C = B * Fr * S, 320
    t = torch.empty(M, C, dtype=EL, device=DEV)
    ops.layernorm(g0h, ln[0], ln[1], ln[2], t)
    qkv = torch.empty(M, 3 * C, dtype=EL, device=DEV)
    ops.gemm(t, wqkv, qkv, N=3 * C, cin=C)
    a = torch.empty(M, C, dtype=EL, device=DEV)
    ops.attention_temporal(qkv, a, B, Fr, S, C)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    ops.gemm(a, wop, hi, out_lo=lo, N=C, cin=C, bias=bias, R1=g0h, R1_lo=g0l, **vkw)
    return hi, lo


@pytest.mark.parametrize("data", ["natural", "lo_only_1", "lo_only_1000"])
@pytest.mark.parametrize("B,Fr,S,vm", [(2, 14, 19, 2), (1, 25, 37, 1)])
def test_temporal_fused_routing_independence(ops, B, Fr, S, vm, data):
    """Split mode: the fused block with its LayerNorm prologue and the four-launch fallback normalise the same input (the hi
    plane of g0) and agree -- on natural data and on rows whose signal is in the lo plane only (where normalising hi + lo on
    one route and hi on the other gives O(1) different branches)."""
    C, M = 320, B * Fr * S
    ws, wqkv, wop, wf = _tf_weights(ops)
    if data == "natural":
        g0h, g0l = split(torch.randn(M, C, generator=g(50)) * 2 + 0.3)
    else:
        g0h, g0l, _ = lo_only_rows(M, C, 1.0 if data == "lo_only_1" else 1000.0, 51)
    bias = torch.randn(C, generator=g(52)).to(DEV)
    vt = torch.randn(B, C, generator=g(53))
    vkw = _vkw(vm, vt, B, Fr, S)
    ln = (torch.randn(C, generator=g(54)).to(DEV), (torch.randn(C, generator=g(55)) * 0.1).to(DEV), 1e-5)
    g0h, g0l = g0h.to(DEV), g0l.to(DEV)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    assert ops.temporal_fused_serves(g0h, wf, hi, B, Fr, S, out_lo=lo, R1=g0h, R1_lo=g0l, ln=ln, **vkw)
    ops.temporal_fused(g0h, wf, hi, B, Fr, S, bias=bias, R1=g0h, R1_lo=g0l, out_lo=lo, ln=ln, **vkw)
    fh, fl = _fallback(ops, g0h, g0l, wqkv, wop, ln, bias, B, Fr, S, vkw)
    trunk = g0h.cpu().double() + decode_lo(g0l.cpu())
    br_fused = hi.cpu().double() + decode_lo(lo.cpu()) - trunk
    br_fall = fh.cpu().double() + decode_lo(fl.cpu()) - trunk
    # (the branch alone: the same bound as the fused block against its launches, tests/test_ops_gpu.py test_temporal_fused)
    assert rel_l2(br_fused, br_fall) < 3e-3, data


def test_temporal_fused_lo_full_size(ops):
    """2 x 25 frames x 72 x 128 pixels, C = 320, split: bit-stable run to run, a clip's bits in the B = 2 launch equal the
    B = 1 launch, and per element (check_split) against fp64 on ~2 000 sampled pixels plus the first pixel, the last pixel
    and the pixels of the last 8-pixel group."""
    B, Fr, S, C = 2, 25, 72 * 128, 320
    M = B * Fr * S
    ws, _, _, wf = _tf_weights(ops, wo_scale=0.05)
    x = torch.randn(M, C, generator=g(60)).to(EL)
    r1h, r1l = split(torch.randn(M, C, generator=g(61)) * 4 + 96)
    bias = torch.randn(C, generator=g(62)) * 0.1
    vt = torch.randn(B, C, generator=g(63)) * 0.1
    kw = dict(bias=bias.to(DEV), R1=r1h.to(DEV), R1_lo=r1l.to(DEV), **_vkw(1, vt, B, Fr, S))
    xd = x.to(DEV)
    hi, lo = torch.full((M, C), float("nan"), dtype=EL, device=DEV), lo_plane(M, C)
    ops.temporal_fused(xd, wf, hi, B, Fr, S, out_lo=lo, **kw)
    hi2, lo2 = torch.full_like(hi, float("nan")), lo_plane(M, C)
    ops.temporal_fused(xd, wf, hi2, B, Fr, S, out_lo=lo2, **kw)
    assert_planes_equal(hi2, lo2, hi.cpu(), lo.cpu().view(torch.uint8), "full size, run to run")
    M1 = Fr * S
    h1, l1 = torch.full((M1, C), float("nan"), dtype=EL, device=DEV), lo_plane(M1, C)
    ops.temporal_fused(xd[M1:].contiguous(), wf, h1, 1, Fr, S, out_lo=l1, bias=bias.to(DEV), R1=r1h[M1:].to(DEV),
                       R1_lo=r1l[M1:].to(DEV), V=vt[1:].float().to(DEV), vmode=1, vdiv=Fr * S)
    assert_planes_equal(h1, l1, hi[M1:].cpu(), lo[M1:].cpu().view(torch.uint8), "clip 1 alone vs in the batch")
    npix = B * S
    pix = torch.randperm(npix, generator=g(64))[:2000]
    pix = torch.unique(torch.cat([pix, torch.tensor([0, npix - 1]), torch.arange((npix - 1) // 8 * 8, npix)]))
    b, s = pix // S, pix % S
    rows = ((b[:, None] * Fr + torch.arange(Fr)[None, :]) * S + s[:, None]).reshape(-1)   # (pixel, frame) rows
    P = pix.numel()
    # the sampled pixels as a batch of one clip of P pixels: attention is independent per pixel
    xs = x[rows].reshape(P, Fr, C).permute(1, 0, 2).reshape(Fr * P, C).double()
    rs = r1h[rows].reshape(P, Fr, C).permute(1, 0, 2).reshape(Fr * P, C).double()
    v64, err = _tf_reference(xs, ws, bias, rs, 1, Fr, P)
    v64 = v64.reshape(Fr, P, C).permute(1, 0, 2).reshape(-1, C) + vt.double()[b].repeat_interleave(Fr, 0)
    err = err.reshape(Fr, P, C).permute(1, 0, 2).reshape(-1, C)
    v64 = v64 + decode_lo(r1l[rows])
    check_split(hi.cpu()[rows], lo.cpu()[rows], v64, err, "full size, sampled pixels")
