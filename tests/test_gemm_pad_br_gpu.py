"""GPU tests of the gather-GEMM's bottom / right padded stride-2 mode (`pad_br`: the VAE encoder's down-samplers,
`F.pad(x, (0, 1, 0, 1))` + Conv2d(3, stride 2, padding 0)), of `ctrlv_vae_posterior`, and of the encoder walk that uses both.

Bounds (tests/test_ops_gpu.py): bf16 operands, fp32 accumulation, one bf16 rounding of the result -> parity_err < 3e-3 against
fp32 PyTorch on the same bf16-rounded inputs; fp32 outputs < 1e-5 (the posterior is a 2L-term fp32 sum per value: nothing
but fp32 rounding); the VAE walk < 2.5e-2 against the CPU oracle (tests/test_vae_gpu.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.parity_utils import parity_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
# every tile id tests/test_ops_gpu.py runs a stride-2 conv on (test_gemm_conv3x3: 1-6, 10; test_gemm_w16_conv3x3: 12, 13), and
# the dispatcher's own choice
TILES = [0, 1, 2, 3, 4, 5, 6, 10, 12, 13]
SHAPES = {"edges": (3, 64, 96, 8, 12),       # last row / column of every image hit the padding, images end inside a tile
          "vae": (2, 128, 128, 16, 16),      # the widths of the encoder's first down-sampler
          "w16_256": (5, 64, 256, 16, 24),   # the shape test_gemm_w16_conv3x3 runs tiles 12 / 13 at: wave tiles with every
          "w16_320": (5, 64, 320, 16, 24)}   # column in use (at N = 96 / 128 most of a 256 / 320-wide tile is masked)


def g(seed):
    return torch.Generator().manual_seed(seed)


def rows_from_nchw(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cases(ops):
    """Per shape: inputs on the device and the fp32 reference rows, computed once."""
    from ctrlv_amd import packing
    out = {}
    for name, (n, cin, cout, H, W) in SHAPES.items():
        x = torch.randn(n, cin, H, W, generator=g(1)).to(BF)
        wt = torch.randn(cout, cin, 3, 3, generator=g(2)) / math.sqrt(9 * cin)
        b = torch.randn(cout, generator=g(3))
        ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.to(BF).float(), b, stride=2)
        assert ref.shape == (n, cout, H // 2, W // 2)
        M = n * (H // 2) * (W // 2)
        out[name] = dict(n=n, cin=cin, cout=cout, H=H, W=W, M=M, ref=rows_from_nchw(ref), xd=rows_from_nchw(x).to(DEV),
                         wd=packing.pack_conv3x3(wt).to(DEV), bd=b.to(DEV),
                         R1=torch.randn(M, cout, generator=g(4)).to(BF), V=torch.randn(n, cout, generator=g(5)))
    return out


def _run(ops, c, tile, stride1=False, **kw):
    H, W = c["H"], c["W"]
    Ho, Wo = (H, W) if stride1 else (H // 2, W // 2)
    out = torch.full((c["n"] * Ho * Wo, c["cout"]), float("nan"), dtype=BF, device=DEV)
    ops.gemm(c["xd"], c["wd"], out, N=c["wd"].shape[0], cin=c["cin"], taps=9, mode=1,
             conv=(H, W, Ho, Wo, 1 if stride1 else 2, 0), bias=c["bd"], n_store=c["cout"], tile=tile,
             pad_br=not stride1, **kw)
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape", ["edges", "vae"])
def test_pad_br_conv(ops, cases, shape, tile):
    """T1: against F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2), plain, with an R1 residual and with a V row vector; and,
    on the same tile id, bit for bit the odd positions of the stride-1 conv (these row widths are below the row-halo
    kernels' 32: both launches sum in tap-major order, the products of an output element are the same sequence)."""
    _check_pad_br(ops, cases[shape], shape, tile)


@pytest.mark.parametrize("shape,tile", [("w16_256", 12), ("w16_320", 13)])
def test_pad_br_conv_full_w16_tiles(ops, cases, shape, tile):
    """The same checks at the shape test_gemm_w16_conv3x3 runs the 16x16x32 core at (every column of its wave tiles in use)."""
    _check_pad_br(ops, cases[shape], shape, tile)


def _check_pad_br(ops, c, shape, tile):
    n, H, W, M, cout = c["n"], c["H"], c["W"], c["M"], c["cout"]
    out = _run(ops, c, tile)
    assert parity_err(out.cpu(), c["ref"], f"pad_br {shape} tile {tile}") < 3e-3
    r1 = _run(ops, c, tile, R1=c["R1"].to(DEV), s1=0.5, s_acc=0.75)
    assert parity_err(r1.cpu(), 0.75 * c["ref"] + 0.5 * c["R1"].float(), "  + R1") < 3e-3
    v = _run(ops, c, tile, V=c["V"].to(DEV), vmode=1, vdiv=(H // 2) * (W // 2))
    assert parity_err(v.cpu(), c["ref"] + c["V"][torch.arange(M) // ((H // 2) * (W // 2))], "  + V") < 3e-3
    full = _run(ops, c, tile, stride1=True)
    odd = full.view(n, H, W, cout)[:, 1::2, 1::2].reshape(M, cout)
    assert not (W >= 32 and 256 % W == 0), "row-halo geometry: the stride-1 launch would sum in another K order"
    assert torch.equal(out, odd)


def test_pad_br_leaves_the_symmetric_stride_2_conv_alone(ops, cases):
    """pad_br = 0 is the padding-1 conv it always was (and differs from pad_br = 1: the two read different pixels)."""
    c = cases["edges"]
    n, H, W = c["n"], c["H"], c["W"]
    sym = torch.empty(c["M"], c["cout"], dtype=BF, device=DEV)
    ops.gemm(c["xd"], c["wd"], sym, N=c["wd"].shape[0], cin=c["cin"], taps=9, mode=1, conv=(H, W, H // 2, W // 2, 2, 0),
             bias=c["bd"], n_store=c["cout"])
    full = _run(ops, c, 0, stride1=True)
    assert torch.equal(sym, full.view(n, H, W, -1)[:, 0::2, 0::2].reshape(c["M"], -1))
    assert not torch.equal(sym, _run(ops, c, 0))


# ---------------------------------------------------------------------------------------------- ctrlv_vae_posterior (T2)
def _posterior_inputs():
    n, L, h, w = 2, 4, 8, 8
    rows = (torch.randn(n * h * w, 2 * L, generator=g(7)) * 3).to(BF)
    qw = torch.randn(2 * L, 2 * L, generator=g(8)) / math.sqrt(2 * L)
    qb = torch.randn(2 * L, generator=g(9))
    qb[L:] += torch.tensor([40.0, -60.0, 0.0, 0.0])          # log-variances outside [-30, 20]: the clamp acts
    noise = torch.randn(n, L, h, w, generator=g(10))
    q = (rows.float() @ qw.t() + qb).view(n, h, w, 2 * L).permute(0, 3, 1, 2).contiguous()      # quant_conv as a matmul
    mean, logvar = torch.chunk(q, 2, dim=1)
    assert (logvar > 20).any() and (logvar < -30).any()
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    return n, L, h, w, rows, qw, qb, noise, q, mean, std


@pytest.mark.parametrize("dtype,bound", [(BF, 3e-3), (torch.float32, 1e-5)])
def test_vae_posterior(ops, dtype, bound):
    n, L, h, w, rows, qw, qb, noise, q, mean, std = _posterior_inputs()
    scale = 0.18215
    rd, qwd, qbd, nd = rows.to(DEV), qw.to(DEV), qb.to(DEV), noise.to(DEV)
    new = lambda c: torch.full((n, c, h, w), float("nan"), dtype=dtype, device=DEV)      # noqa: E731
    # with noise, both outputs
    mom, lat = ops.vae_posterior(rd, n, L, h * w, qwd, qbd, nd, scale, new(2 * L), new(L))
    assert parity_err(mom.cpu(), q, f"moments {dtype}") < bound
    assert parity_err(lat.cpu(), scale * (mean + std * noise), f"latents, sampled {dtype}") < bound
    # mode(): no noise
    _, lat0 = ops.vae_posterior(rd, n, L, h * w, qwd, qbd, None, scale, None, new(L))
    assert parity_err(lat0.cpu(), scale * mean, f"latents, mode {dtype}") < bound
    # moments only / latents only give the same bits as the joint call, and so does a second run
    mom1, _ = ops.vae_posterior(rd, n, L, h * w, qwd, qbd, None, 1.0, new(2 * L), None)
    _, lat1 = ops.vae_posterior(rd, n, L, h * w, qwd, qbd, nd, scale, None, new(L))
    mom2, lat2 = ops.vae_posterior(rd, n, L, h * w, qwd, qbd, nd, scale, new(2 * L), new(L))
    assert torch.equal(mom1, mom) and torch.equal(lat1, lat) and torch.equal(mom2, mom) and torch.equal(lat2, lat)
    # a wider row pitch (ld > 2 L) reads the same values
    wide = torch.zeros(n * h * w, 16, dtype=BF, device=DEV)
    wide[:, :2 * L] = rd
    mom3, lat3 = ops.vae_posterior(wide, n, L, h * w, qwd, qbd, nd, scale, new(2 * L), new(L))
    assert torch.equal(mom3, mom) and torch.equal(lat3, lat)


# ------------------------------------------------------------------------------- the encoder walk on the two kernels (T5)
@pytest.fixture(scope="module")
def vae(hip_lib):
    """The construction of tests/test_vae_gpu.py: production widths, mix factors 0.4, bf16-rounded parameters."""
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder
    torch.manual_seed(5)
    m = AutoencoderKLTemporalDecoder().eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(0.4)
            p.copy_(p.to(BF).float())
    return m


@pytest.mark.parametrize("n,H,W", [(2, 128, 192), (1, 64, 64)])
def test_vae_encode_native_down(vae, n, H, W):
    """`encode(native_down=True)` (one pad_br launch per down-sampler) against the CPU oracle's pre-quant_conv moments, and
    `ctrlv_vae_posterior` on its conv_out rows against the oracle's post-quant_conv moments: the mean half times the scaling
    factor for mode(), mean + std * noise for a given noise tensor.  The default route's error is printed beside."""
    import copy
    import ctrlv_ref as R
    from ctrlv_amd import ops
    from ctrlv_amd.models import vae_encoder_hip as ve
    x = (torch.rand(n, 3, H, W, generator=g(4)) * 2 - 1).to(BF).float()
    sd = {k: v.detach() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        ref_pre = R.vae.encode_moments(sd, x, quant=False)
        ref_q = R.vae.encode_moments(sd, x)
    dev_vae = copy.deepcopy(vae).to(DEV, BF)
    xd = x.to(DEV, BF)
    sf = dev_vae.config.scaling_factor
    h, w = H // 8, W // 8
    noise = torch.randn(n, 4, h, w, generator=g(6))
    qw = dev_vae.quant_conv.weight.detach().float().reshape(8, 8).contiguous()
    qb = dev_vae.quant_conv.bias.detach().float().contiguous()
    new = lambda c: torch.empty(n, c, h, w, dtype=BF, device=DEV)      # noqa: E731
    with torch.no_grad():
        twin = ve.encode(dev_vae.encoder, xd, native_down=True)
        default = ve.encode(dev_vae.encoder, xd)
        rows = ve.encode(dev_vae.encoder, xd, native_down=True, rows=True)
        mom, lat = ops.vae_posterior(rows, n, 4, h * w, qw, qb, None, sf, new(8), new(4))
        _, lat_n = ops.vae_posterior(rows, n, 4, h * w, qw, qb, noise.to(DEV), sf, None, new(4))
        again = ve.encode(dev_vae.encoder, xd, native_down=True)
    torch.cuda.synchronize()
    parity_err(default.float().cpu(), ref_pre, "default route (stride-1 conv + strided copy)")
    assert twin.shape == (n, 8, h, w) and twin.dtype == BF
    assert parity_err(twin.float().cpu(), ref_pre, "native_down moments") < 2.5e-2
    assert torch.equal(twin, again)
    mean, logvar = torch.chunk(ref_q, 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    assert parity_err(mom.float().cpu(), ref_q, "moments after quant_conv") < 2.5e-2
    assert parity_err(lat.float().cpu(), sf * mean, "latents (mode)") < 2.5e-2
    assert parity_err(lat_n.float().cpu(), sf * (mean + std * noise), "latents (mean + std * noise)") < 2.5e-2
