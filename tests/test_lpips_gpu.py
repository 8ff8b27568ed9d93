"""LPIPS on the device (csrc/lpips.hip) with bf16 elements; tests/test_lpips_f16_gpu.py runs this file again with fp16 elements.

Exact where the arithmetic is: the split im2col rows, the packed weights and the pool are compared bit for bit with their torch
construction.  One layer (im2col + ctrlv_gemm) is held to the worst-case bound of an fp32-accumulated sum of exact products
against the emulation of tests/lpips_ref.py; the distance kernel to the sequential-sum bound against fp64; the metric to
4 x (a + b) of fp64, a and b being the emulation's and the fp32 torch forward's own worst errors on the test's pairs, computed
here on the CPU -- never a number taken from the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ctrlv_amd.models.lpips_alex import CONVS, SCALE, SHIFT, LpipsAlexWeights, split_weight_columns
from tests import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EL = torch.bfloat16                  # (tests/test_lpips_f16_gpu.py rebinds this; read at call time)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


@pytest.fixture(scope="module")
def weights():
    return LpipsAlexWeights.random(0)


@pytest.fixture(scope="module")
def lpips_plan(hip_lib, weights):
    from ctrlv_amd.plan import LpipsPlan
    return LpipsPlan(weights, DEV, dtype=EL)


def _split_rows(cols, kp):
    """fp32 (M, K) -> element rows (M, 3 Kp) = lo | hi | hi with zero padding columns, built in torch on the CPU."""
    full = torch.zeros(cols.shape[0], kp, dtype=torch.float32)
    full[:, :cols.shape[1]] = cols
    hi, lo = R.split(full, EL)
    return torch.cat([lo, hi, hi], dim=1)


# ---------------------------------------------------------------------------------------------------------------- exact kernels
@pytest.mark.parametrize("src", ["uint8", "fp32"])
def test_im2col_first_layer_bit_for_bit(hip_lib, src):
    """37 x 50: (H - 7) is no multiple of 4, the windows of the first and last rows / columns hang over all four borders."""
    from ctrlv_amd import ops
    g = torch.Generator().manual_seed(11)
    m, H, W = 2, 37, 50
    if src == "uint8":
        frames = torch.randint(0, 256, (m, 3, H, W), generator=g, dtype=torch.uint8)
        unit = R.frames_to_unit(frames, torch.float32)
    else:
        frames = unit = torch.rand(m, 3, H, W, generator=g) * 2 - 1
    x = R.scaling_layer(unit)
    cols = F.unfold(x, 11, padding=2, stride=4)                       # (m, 363, 8 * 11) in (c, ky, kx) order
    assert cols.shape[2] == 8 * 11
    want = _split_rows(cols.permute(0, 2, 1).reshape(m * 88, 363), 384)
    got = ops.lpips_im2col_split(frames.to(DEV), dtype=EL).cpu()
    assert got.dtype == EL and tuple(got.shape) == (m * 88, 3 * 384)
    assert torch.equal(_bits(got), _bits(want))
    assert not got[:, 363:384].any() and not got[:, 384 + 363:768].any() and not got[:, 768 + 363:].any()
    assert bool(got[:, :363].any())                                   # lo is not trivially zero
    assert torch.equal(_bits(got[:, 384:768].contiguous()), _bits(got[:, 768:].contiguous()))       # hi twice


@pytest.mark.parametrize("hw", [(3, 5), (1, 2)])
@pytest.mark.parametrize("C,k", [(64, 5), (192, 3), (384, 3), (256, 3)])
def test_im2col_rows_form_bit_for_bit(hip_lib, C, k, hw):
    """ReLU on read, tap-major (ky, kx, c) columns, zero taps at every border (a 5 x 5 window on 3 x 5 pixels leaves them on all
    four sides of every pixel), from a pitched source."""
    from ctrlv_amd import ops
    g = torch.Generator().manual_seed(C + k)
    m, (H, W) = 2, hw
    wide = torch.randn(m * H * W, C + 8, generator=g)
    rows = wide[:, :C]
    x = torch.relu(rows).reshape(m, H, W, C).permute(0, 3, 1, 2)
    cols = F.unfold(x, k, padding=(k - 1) // 2).reshape(m, C, k * k, H * W).permute(0, 3, 2, 1).reshape(m * H * W, k * k * C)
    kp = ops.lpips_kp(C, k)
    want = _split_rows(cols, kp)
    got = ops.lpips_im2col_split(wide.to(DEV)[:, :C], k=k, hw=(m, H, W), dtype=EL).cpu()
    assert tuple(got.shape) == (m * H * W, 3 * kp)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("l", range(5))
def test_packed_weights_bit_for_bit(hip_lib, weights, l):
    from ctrlv_amd import ops
    w, _ = weights.conv(l)
    order = 0 if l == 0 else 1
    got = ops.lpips_pack_weight(w.to(DEV), order, dtype=EL).cpu()
    assert torch.equal(_bits(got), _bits(split_weight_columns(w, order, EL)))


@pytest.mark.parametrize("hw", [(8, 11), (3, 5)])
def test_relu_maxpool_rows_bit_for_bit(hip_lib, hw):
    """8 x 11 -> 3 x 5 and 3 x 5 -> 1 x 2: floor mode drops a row or a column in each; a window of negatives gives 0."""
    from ctrlv_amd import ops
    g = torch.Generator().manual_seed(5)
    m, (H, W), C = 2, hw, 64
    x = torch.randn(m * H * W, C, generator=g)
    first = [y * W + c for y in range(3) for c in range(3)]           # the first window of image 0 is all negative
    x[first] = -x[first].abs()
    want = F.max_pool2d(torch.relu(x.reshape(m, H, W, C).permute(0, 3, 1, 2)), 3, 2)
    Ho, Wo = want.shape[2:]
    assert (Ho, Wo) == ((H - 3) // 2 + 1, (W - 3) // 2 + 1) and not want[0, :, 0, 0].any()
    got = ops.relu_maxpool_rows(x.to(DEV), (m, H, W)).cpu()
    assert torch.equal(got, want.permute(0, 2, 3, 1).reshape(m * Ho * Wo, C))


# ---------------------------------------------------------------------------------------------------------------- one layer
def _layer_input(l, m, g):
    """The input of convolution l at the sizes of the 37 x 50 chain: frames for l = 0, else fp32 rows (pre-ReLU)."""
    sizes = [(37, 50), (3, 5), (1, 2), (1, 2), (1, 2)]
    H, W = sizes[l]
    if l == 0:
        return torch.randint(0, 256, (m, 3, H, W), generator=g, dtype=torch.uint8), H, W
    return torch.randn(m * H * W, CONVS[l][1], generator=g), H, W


@pytest.mark.parametrize("l", range(5))
def test_one_layer_against_the_emulated_convolution(hip_lib, weights, l):
    """im2col + ctrlv_gemm (fp32 output, the 128 x 128 tile) against hi whi + lo whi + hi wlo + b summed in fp64 and rounded once:
    |y - y_emu| <= 2 K 2^-24 (|x| (*) |w| + |b|), K = 3 Kp -- the worst case of an fp32-accumulated sum of K exact products."""
    from ctrlv_amd import ops
    g = torch.Generator().manual_seed(20 + l)
    _, cin, cout, k, stride, pad = CONVS[l]
    m = 3
    src, H, W = _layer_input(l, m, g)
    w, b = weights.conv(l)
    if l == 0:
        x = R.scaling_layer(R.frames_to_unit(src, torch.float32))
        A = ops.lpips_im2col_split(src.to(DEV), dtype=EL)
    else:
        x = torch.relu(src).reshape(m, H, W, cin).permute(0, 3, 1, 2)
        A = ops.lpips_im2col_split(src.to(DEV), k=k, hw=(m, H, W), dtype=EL)
    Wp = ops.lpips_pack_weight(w.to(DEV), 0 if l == 0 else 1, dtype=EL)
    out = torch.empty(A.shape[0], cout, dtype=torch.float32, device=DEV)
    ops.gemm(A, Wp, out, N=cout, cin=A.shape[1], bias=b.to(DEV), out_f32=True, tile=1, splitk=False)
    y_emu = R.conv_split(x, w, b, EL, stride, pad)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad) + b.double().abs().reshape(1, -1, 1, 1)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, cout)          # noqa: E731
    assert out.shape[0] == rows(y_emu).shape[0]
    err = (out.cpu().double() - rows(y_emu).double()).abs()
    bound = 2.0 * A.shape[1] * 2.0 ** -24 * rows(mag)
    print(f"layer {l}: worst |y - y_emu| / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------------------- distance
@pytest.mark.parametrize("pix", [1, 2, 15, 88])
@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_layer_distance_against_fp64(hip_lib, C, pix):
    """Independent N(0, 1) rows (no cancellation); relative error of a frame's mean distance <= 4 (C + 8) 2^-24, the bound of a
    sequential fp32 sum of C terms with the few operations around it, so it holds for any reduction tree."""
    from ctrlv_amd import ops
    g = torch.Generator().manual_seed(C + pix)
    frames = 3
    a, b = torch.randn(frames * pix, C, generator=g), torch.randn(frames * pix, C, generator=g)
    lin = torch.rand(C, generator=g) * (2.0 / C)
    part = ops.lpips_layer_distance(a.to(DEV), b.to(DEV), lin.to(DEV), frames)
    assert tuple(part.shape) == (frames, (pix + 63) // 64) and part.dtype == torch.float64
    got = ops.lpips_finish([part], [pix]).cpu()
    ra, rb = torch.relu(a).double(), torch.relu(b).double()
    na = ra / (ra.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = rb / (rb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    want = (lin.double() * (na - nb) ** 2).sum(1).reshape(frames, pix).mean(1)
    rel = ((got - want).abs() / want).max()
    print(f"C={C} pix={pix}: worst relative error {float(rel):.3g}")
    assert float(rel) <= 4 * (C + 8) * 2.0 ** -24
    same = ops.lpips_finish([ops.lpips_layer_distance(a.to(DEV), a.to(DEV), lin.to(DEV), frames)], [pix]).cpu()
    assert same.tolist() == [0.0] * frames                              # identical rows: exactly zero


# ---------------------------------------------------------------------------------------------------------------- the metric
def _tolerance(weights, gt, gen, ref, first=1):
    """(a, b) of the tolerance 4 x (a + b): a = the emulation's, b = the fp32 torch forward's worst relative error against fp64
    over the non-identical pairs (those from `first` on) -- both formed here on the CPU."""
    a = R.rel_err(R.forward_split(weights, gt, gen, EL), ref, first)
    b = R.rel_err(R.forward(weights, gt, gen, torch.float32), ref, first)
    return a, b


@pytest.fixture(scope="module")
def metric_cases(weights):
    """(gt, gen, fp64 reference, a, b) per size; computed once, never changed."""
    cases = {}
    for (H, W, pairs) in ((37, 50, 6), (64, 96, 4)):
        gt, gen = R.make_pairs(H, W, pairs, seed=H)
        ref = R.forward(weights, gt, gen)
        cases[(H, W)] = (gt, gen, ref) + _tolerance(weights, gt, gen, ref)
    return cases


@pytest.mark.parametrize("size", [(37, 50), (64, 96)])
def test_metric_within_four_times_the_cpu_forwards_own_error(lpips_plan, weights, metric_cases, size):
    gt, gen, ref, a, b = metric_cases[size]
    got = lpips_plan.frames(gt[None].to(DEV), gen[None].to(DEV)).cpu()[0]
    assert got.dtype == torch.float64 and float(got[0]) == 0.0 and float(ref[0]) == 0.0       # the identical pair: exactly 0
    rel = ((got - ref).abs() / ref.abs())[1:]
    print(f"{size} {EL}: a = {a:.3g}, b = {b:.3g}, device worst = {float(rel.max()):.3g} (per pair {[f'{v:.2g}' for v in rel.tolist()]})")
    assert bool((rel <= 4 * (a + b)).all())
    # the reason the split exists: plain 16-bit storage is at least 16 times worse on the pair one grey level apart
    plain = R.forward_plain16(weights, gt[:2], gen[:2], EL)
    plain_rel = abs(float(plain[1] - ref[1])) / float(ref[1])
    print(f"{size} {EL}: plain 16-bit forward on the +-1 pair {plain_rel:.3g}")
    assert plain_rel >= 16 * float(rel[0])


def test_fp32_frames_take_the_same_path(lpips_plan, weights, metric_cases):
    """fp32 frames in [-1, 1] skip only the u8 conversion: on the values u8 / 127.5 - 1 the bits are those of the uint8 call."""
    gt, gen, *_ = metric_cases[(37, 50)]
    u8 = lpips_plan.frames(gt[None].to(DEV), gen[None].to(DEV))
    f32 = lpips_plan.frames(R.frames_to_unit(gt, torch.float32)[None].to(DEV), R.frames_to_unit(gen, torch.float32)[None].to(DEV))
    assert torch.equal(u8, f32)


def test_a_frames_bits_do_not_depend_on_batch_chunk_or_workspace(lpips_plan, metric_cases):
    gt, gen, *_ = metric_cases[(37, 50)]
    gt, gen = gt.to(DEV), gen.to(DEV)
    base = lpips_plan.frames(gt[None], gen[None])                              # (1, 6)
    assert torch.equal(lpips_plan.frames(gt[None], gen[None]), base)           # a second call
    two = lpips_plan.frames(gt.reshape(2, 3, 3, 37, 50), gen.reshape(2, 3, 3, 37, 50))
    assert torch.equal(two.reshape(-1), base.reshape(-1))
    one = lpips_plan.frames(gt[None, 3:4], gen[None, 3:4])                     # (1, 1)
    assert torch.equal(one.reshape(-1), base[0, 3:4])
    # a workspace that holds one frame pair at a time against one that holds all six
    small = torch.empty(lpips_plan.workspace_bytes(37, 50, 1), dtype=torch.uint8, device=DEV)
    large = torch.empty(lpips_plan.workspace_bytes(37, 50, 6) + 4096, dtype=torch.uint8, device=DEV)
    assert small.numel() < lpips_plan.workspace_bytes(37, 50, 2)
    assert torch.equal(lpips_plan.frames(gt[None], gen[None], workspace=small), base)
    assert torch.equal(lpips_plan.frames(gt[None], gen[None], workspace=large), base)
    four = torch.empty(lpips_plan.workspace_bytes(37, 50, 4), dtype=torch.uint8, device=DEV)
    assert four.numel() < lpips_plan.workspace_bytes(37, 50, 5)
    assert torch.equal(lpips_plan.frames(gt[None], gen[None], workspace=four), base)          # chunks of 4 + 2


def test_the_evaluations_size_through_metrics(lpips_plan, weights):
    """Two frames of 320 x 512 uint8 resized as PIL does to 256 x 410, as evaluate_vids does, through metrics.lpips_frames; same
    bound, the reference from the same resized frames."""
    from ctrlv_amd import metrics, ops
    g = torch.Generator().manual_seed(9)
    gt = torch.randint(40, 216, (2, 3, 320, 512), generator=g, dtype=torch.int16)
    gen = gt.clone()
    gen[0] += torch.randint(0, 2, (3, 320, 512), generator=g, dtype=torch.int16) * 2 - 1
    gen[1] += torch.randint(-40, 41, (3, 320, 512), generator=g, dtype=torch.int16)
    gt, gen = gt.to(torch.uint8).to(DEV), gen.to(torch.uint8).to(DEV)
    got = metrics.lpips_frames(gt, gen, lpips_plan, size=(256, 410))
    assert got.dtype == np.float64 and got.shape == (2,)
    both = metrics.frame_quality(gt, gen, size=(256, 410), lpips=lpips_plan)
    assert np.array_equal(both["lpips"], got) and set(both) == {"ssim", "psnr", "lpips"}
    assert metrics.quality_summary(both["ssim"], both["psnr"], lpips=both["lpips"])["lpips_score"] == float(got.mean())
    rg, rn = ops.resize_frames_u8(gt, 256, 410).cpu(), ops.resize_frames_u8(gen, 256, 410).cpu()
    ref = R.forward(weights, rg, rn)
    a, b = _tolerance(weights, rg, rn, ref, first=0)
    rel = (torch.from_numpy(got) - ref).abs() / ref
    print(f"256 x 410 {EL}: a = {a:.3g}, b = {b:.3g}, device {[f'{v:.2g}' for v in rel.tolist()]}")
    assert bool((rel <= 4 * (a + b)).all())


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_refusals(lpips_plan):
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)              # noqa: E731
    with pytest.raises(ValueError, match="31 x 31.*status -2"):
        lpips_plan.frames(z(1, 1, 3, 30, 50), z(1, 1, 3, 30, 50))
    with pytest.raises(ValueError, match="31 x 31.*status -2"):
        lpips_plan.frames(z(1, 1, 3, 50, 30), z(1, 1, 3, 50, 30))
    short = torch.empty(lpips_plan.workspace_bytes(37, 50, 1) - 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="status -5"):
        lpips_plan.frames(z(1, 2, 3, 37, 50), z(1, 2, 3, 37, 50), workspace=short)
    with pytest.raises(ValueError, match="gen must be"):
        lpips_plan.frames(z(1, 2, 3, 37, 50), z(1, 2, 3, 37, 51))
    with pytest.raises(ValueError, match="gen must be"):
        lpips_plan.frames(z(1, 2, 3, 37, 50), z(1, 2, 3, 37, 50).float())
    from ctrlv_amd import metrics
    with pytest.raises(ValueError, match="gen must be"):
        metrics.lpips_frames(z(2, 3, 37, 50), z(3, 3, 37, 50), lpips_plan)
