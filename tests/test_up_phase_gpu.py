"""The nearest-x2 upsampler conv in PHASE FORM (ctrlv_gemm_desc.up = 2, csrc/gemm_pp_up.hip): four 2x2 convs on the
low-resolution input, one per output parity, against the 3x3 gather over the upsampled grid (up = 1) and PyTorch.

  * exact placement: small-integer inputs, weights and bias make every product, every presummed phase weight and every fp32
    sum exact, so the two launches and F.conv2d(F.interpolate(...)) must agree bit for bit -- any tap, phase, border or
    row-remap error shows;
  * rounding: the phase weight is a sum of 1, 2, 2 or 4 taps rounded ONCE to the element type -- one more independent
    rounding of the size of the output rounding, predicted error ratio sqrt(2) against the fp64 conv of the parameter;
  * clip independence and routing (the layer's shape decides, never the image count).
Both element libraries (bf16, fp16)."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests.parity_utils import parity_err, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELS = [torch.bfloat16, torch.float16]
LO = torch.float8_e5m2        # the lo plane of a split trunk tensor: one byte per element (fp16 library)

# (n_img, H, W, Cin, N): 144 input pixels = one ragged tile per phase with image borders inside it; 576 = 2.25 tiles per
# phase; one image row = every tap row out of range on one side
SHAPES = [(3, 3, 16, 64, 64), (2, 9, 32, 64, 320), (1, 1, 16, 64, 64)]


def tol(bf16_bound, el):
    """tests/test_ops_gpu.py tol(): the stated bf16 bound, a sixth of it for fp16 outputs"""
    return bf16_bound if el == torch.bfloat16 else bf16_bound / 6.0


@pytest.fixture(scope="module")
def ops(hip_lib):
    from ctrlv_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def rows_from_nchw(x):
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def nchw_from_rows(r, n, h, w):
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


def launch(ops, el, x, wt, b, up, out_lo=False):
    """x (n, C, H, W) and the parameter wt [N, C, 3, 3] (CPU tensors) -> output rows [n 4HW, N] (and the lo plane)"""
    from ctrlv_amd import packing
    n, cin, H, W = x.shape
    cout = wt.shape[0]
    if up == 2:
        wd = ops.pack_up_phase_weight(wt.to(DEV), el)
    else:
        with packing.element_dtype(el):
            wd = packing.pack_conv3x3(wt).to(DEV)
    out = torch.full((n * 4 * H * W, cout), float("nan"), dtype=el, device=DEV)
    lo = torch.empty(n * 4 * H * W, cout, dtype=LO, device=DEV) if out_lo else None
    if lo is not None:
        lo.view(torch.uint8).fill_(0x7F)
    kw = dict(N=cout, cin=cin, taps=9, mode=1, bias=b.to(DEV), out_lo=lo)
    xd = rows_from_nchw(x).to(el).to(DEV)
    if up == 2:
        assert ops.gemm_up_phase_serves(xd, wd, out, conv=(H, W, 2 * H, 2 * W, 1, 1), **kw)
    ops.gemm(xd, wd, out, conv=(H, W, 2 * H, 2 * W, 1, up), **kw)
    return (out, lo) if out_lo else out


def phase_convs_f64(x, wph, b):
    """the four 2x2 convs of the packed panels wph [4, N, 4 C] (include/ctrlv_hip.h up = 2) in fp64, x (n, C, H, W)"""
    n, C, H, W = x.shape
    N = wph.shape[1]
    xp = F.pad(x.double(), (1, 1, 1, 1))
    out = torch.empty(n, N, 2 * H, 2 * W, dtype=torch.float64)
    for p in range(4):
        py, px = p >> 1, p & 1
        w = wph[p].double().reshape(N, 2, 2, C).permute(0, 3, 1, 2)         # [N, C, a, b]
        out[:, :, py::2, px::2] = F.conv2d(xp, w, b.double())[:, :, py:py + H, px:px + W]
    return out


@pytest.mark.parametrize("el", ELS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,H,W,cin,cout", SHAPES)
def test_exact_placement(ops, el, n, H, W, cin, cout):
    x = torch.randint(-4, 5, (n, cin, H, W), generator=g(1)).float()
    wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g(2)).float()
    b = torch.randint(-8, 9, (cout,), generator=g(3)).float()
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), b.double(), padding=1)
    assert float(ref.abs().max()) < 2 ** 24              # every fp32 partial sum is exact
    ref = rows_from_nchw(ref).to(el)
    new = launch(ops, el, x, wt, b, 2).cpu()
    old = launch(ops, el, x, wt, b, 1).cpu()
    assert torch.equal(old, ref), "the up = 1 launch"
    bad = (new != ref).any(dim=1).nonzero().flatten()
    assert torch.equal(new, ref), f"up = 2: {bad.numel()} rows differ, first {bad[:8].tolist()}"
    assert torch.equal(new, old)


def test_exact_placement_split_planes(ops):
    """fp16 library, split trunk output (hi + lo planes, the form the benchmark's trunk runs in): both planes of the phase
    launch equal those of the up = 1 launch."""
    n, H, W, cin, cout = SHAPES[1]
    x = torch.randint(-4, 5, (n, cin, H, W), generator=g(1)).float()
    wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g(2)).float()
    b = torch.randint(-8, 9, (cout,), generator=g(3)).float()
    hi2, lo2 = launch(ops, torch.float16, x, wt, b, 2, out_lo=True)
    hi1, lo1 = launch(ops, torch.float16, x, wt, b, 1, out_lo=True)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), b.double(), padding=1)
    assert torch.equal(hi2.cpu(), rows_from_nchw(ref).to(torch.float16))
    assert torch.equal(hi2, hi1) and torch.equal(lo2.view(torch.uint8), lo1.view(torch.uint8))


@pytest.mark.parametrize("el", ELS, ids=["bf16", "fp16"])
def test_rounding(ops, el):
    """e_new <= 1.6 e_old against the fp64 conv of the parameter (predicted sqrt(2): one more independent rounding of the size
    of the output rounding; 1.6 leaves room for sampling), and the launch against the fp64 2x2 convs of its own packed
    weights within the bound the conv cases of tests/test_ops_gpu.py apply (tol(3e-3))."""
    n, H, W, cin, cout = SHAPES[1]
    x = torch.randn(n, cin, H, W, generator=g(1)).to(el)
    wt = (torch.randn(cout, cin, 3, 3, generator=g(2)) / math.sqrt(9 * cin)).to(el)     # the parameter, in the element type
    b = torch.randn(cout, generator=g(3))
    ref = rows_from_nchw(F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), b.double(), padding=1))
    new = launch(ops, el, x.float(), wt, b, 2).cpu()
    old = launch(ops, el, x.float(), wt, b, 1).cpu()
    e_new, e_old = rel_l2(new.double(), ref), rel_l2(old.double(), ref)
    print(f"  rel-L2 against the fp64 conv: up = 2 {e_new:.3e}, up = 1 {e_old:.3e}, ratio {e_new / e_old:.3f}")
    assert e_new <= 1.6 * e_old, (e_new, e_old)
    wph = ops.pack_up_phase_weight(wt.to(DEV), el).cpu()
    own = rows_from_nchw(phase_convs_f64(x, wph, b))
    assert parity_err(new, own.float(), "up = 2 against the fp64 2x2 convs of the packed weights") < tol(3e-3, el)


@pytest.mark.parametrize("el", ELS, ids=["bf16", "fp16"])
def test_clip_independence(ops, el):
    n, H, W, cin, cout = SHAPES[1]
    x = torch.randn(n, cin, H, W, generator=g(1)).to(el).float()
    wt = torch.randn(cout, cin, 3, 3, generator=g(2)) / math.sqrt(9 * cin)
    b = torch.randn(cout, generator=g(3))
    both = launch(ops, el, x, wt, b, 2)
    for i in range(n):
        one = launch(ops, el, x[i:i + 1], wt, b, 2)
        assert torch.equal(one, both[i * 4 * H * W:(i + 1) * 4 * H * W]), i


@pytest.mark.parametrize("el", ELS, ids=["bf16", "fp16"])
@pytest.mark.parametrize("W,served", [(12, False), (16, True)])
def test_routing(ops, el, W, served):
    """The executor's up-sampler (models/blocks.py Upsample2D, the twin of csrc/plan.hip run_resample) takes the phase form
    where the predicate serves the layer and gives the bits of up = 1 where it refuses (a row width that is no power of
    two)."""
    from ctrlv_amd import packing
    from ctrlv_amd.models.blocks import Upsample2D
    n, H, C = 2, 5, 64
    x = torch.randn(n, C, H, W, generator=g(1)).to(el).float()
    torch.manual_seed(5)
    m = Upsample2D(C).to(DEV)
    with packing.element_dtype(el):
        m.pack()
    ws = types.SimpleNamespace(trunk=lambda shape: torch.full(shape, float("nan"), dtype=el, device=DEV))
    ctx = types.SimpleNamespace(ws=ws, B=n, F=1)
    xd = rows_from_nchw(x).to(el).to(DEV)
    out, Ho, Wo = m.run(ctx, xd, H, W)
    assert (Ho, Wo) == (2 * H, 2 * W)
    probe = torch.empty(n * 4 * H * W, C, dtype=el, device=DEV)
    assert ops.gemm_up_phase_serves(xd, m._pk[0], probe, N=C, cin=C, taps=9, mode=1, bias=m._pk[1],
                                    conv=(H, W, 2 * H, 2 * W, 1, 1)) == served
    want = launch(ops, el, x, m.conv.weight.detach().cpu(), m.conv.bias.detach().cpu(), 2 if served else 1)
    assert torch.equal(out, want)
