"""LPIPS (AlexNet, v0.1) restated in plain torch on the CPU from its published definition, for the tests of csrc/lpips.hip:

    x  = (frame - shift) / scale                      frame in [-1, 1]; shift (-.030, -.088, -.188), scale (.458, .448, .450)
    f1 = relu(conv 3->64, 11x11, stride 4, pad 2)     f2 = relu(conv 64->192, 5x5, pad 2  of maxpool(f1, 3, stride 2))
    f3 = relu(conv 192->384, 3x3, pad 1  of maxpool(f2, 3, 2))    f4 = relu(conv 384->256, 3x3, pad 1 of f3)    f5 likewise, 256->256
    n  = f / (sqrt(sum_c f^2) + 1e-10)                per pixel, for both frames
    score = sum_l mean_pixels( sum_c lin_l[c] (n_gt - n_gen)^2 )

Three forwards over a models.lpips_alex.LpipsAlexWeights:
  forward(..., torch.float64)   the reference
  forward(..., torch.float32)   what a plain fp32 torch forward gives
  forward_split(..., el)        the EMULATION of the kernels' arithmetic: per convolution, x and w split in the element type
                                (hi = rne(x), lo = rne(x - hi)), the three products hi whi + lo whi + hi wlo summed in fp64, the
                                bias added, ONE rounding to fp32; everything between the convolutions in fp32, the per-frame sums
                                in fp64 -- as the device does it, except that the device adds the products in fp32
  forward_plain16(..., el)      activations and weights simply rounded to the element type (what the split is there to avoid)
Frames are (P, 3, H, W) uint8; every forward returns P float64 scores.  No code of the reference or of the `lpips` package."""
import numpy as np
import torch
import torch.nn.functional as F

from ctrlv_amd.models.lpips_alex import CONVS, SCALE, SHIFT


def frames_to_unit(u8, dtype):
    """u8 / 127.5 - 1 in `dtype`, each operation rounded (numpy: IEEE division, no reciprocal)."""
    t = {torch.float32: np.float32, torch.float64: np.float64}[dtype]
    return torch.from_numpy(u8.numpy().astype(t) / t(127.5) - t(1.0))


def scaling_layer(x):
    t = {torch.float32: np.float32, torch.float64: np.float64}[x.dtype]
    shift = np.array(SHIFT, dtype=t).reshape(1, 3, 1, 1)
    scale = np.array(SCALE, dtype=t).reshape(1, 3, 1, 1)
    return torch.from_numpy((x.numpy() - shift) / scale)


def split(x, el):
    """(hi, lo) in the element type: hi = rne(x), lo = rne(x - hi); x fp32."""
    hi = x.to(el)
    lo = (x - hi.float()).to(el)
    return hi, lo


def conv_split(x, w, b, el, stride, pad):
    """The emulated convolution: fp32 x (already ReLU'd) and fp32 w, b -> fp32 y."""
    xh, xl = (t.double() for t in split(x, el))
    wh, wl = (t.double() for t in split(w, el))
    # hi whi + lo whi as one convolution: hi + lo is exact in fp64 (two 16-bit values a few binades apart)
    y = F.conv2d(xh + xl, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad)
    return (y + b.double().reshape(1, -1, 1, 1)).float()


def _features(weights, x, conv):
    """The five pre-ReLU maps of x (scaled input) with `conv(x, w, b, stride, pad)`; ReLU and the pools in x's dtype."""
    outs = []
    for l, (_, _, _, _, stride, pad) in enumerate(CONVS):
        w, b = weights.conv(l)
        y = conv(x, w, b, stride, pad)
        outs.append(y)
        x = torch.relu(y)
        if l < 2:
            x = F.max_pool2d(x, 3, 2)
    return outs


def _score(weights, fg, fn):
    """Per pair: sum over the layers of the pixel mean of sum_c lin (n_gt - n_gen)^2; the pixel arithmetic in the maps' dtype,
    the sums over pixels and layers in fp64."""
    total = torch.zeros(fg[0].shape[0], dtype=torch.float64)
    for l, (a, g) in enumerate(zip(fg, fn)):
        a, g = torch.relu(a), torch.relu(g)
        eps = torch.tensor(1e-10, dtype=a.dtype)
        na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + eps)
        ng = g / (g.pow(2).sum(1, keepdim=True).sqrt() + eps)
        lin = weights.lin(l).to(a.dtype).reshape(1, -1, 1, 1)
        d = (lin * (na - ng) ** 2).sum(1)
        total += d.double().mean(dim=(1, 2))
    return total


def forward(weights, gt_u8, gen_u8, dtype=torch.float64):
    def conv(x, w, b, stride, pad):
        return F.conv2d(x, w.to(dtype), b.to(dtype), stride, pad)
    f = [_features(weights, scaling_layer(frames_to_unit(u, dtype)), conv) for u in (gt_u8, gen_u8)]
    return _score(weights, *f)


def forward_split(weights, gt_u8, gen_u8, el):
    def conv(x, w, b, stride, pad):
        return conv_split(x, w, b, el, stride, pad)
    f = [_features(weights, scaling_layer(frames_to_unit(u, torch.float32)), conv) for u in (gt_u8, gen_u8)]
    return _score(weights, *f)


def forward_plain16(weights, gt_u8, gen_u8, el):
    def conv(x, w, b, stride, pad):
        y = F.conv2d(x.to(el).double(), w.to(el).double(), b.double(), stride, pad)
        return y.float().to(el).float()
    f = [_features(weights, scaling_layer(frames_to_unit(u, torch.float32)), conv) for u in (gt_u8, gen_u8)]
    return _score(weights, *f)


def make_pairs(H, W, pairs, seed):
    """(gt, gen) uint8 (pairs, 3, H, W): pair 0 identical, pair 1 one grey level apart (+-1 per value), the rest +-40 levels
    apart (uniform in [-40, 40]); gt in [40, 215] so that nothing clamps."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(40, 216, (pairs, 3, H, W), generator=g, dtype=torch.int16)
    gen = gt.clone()
    if pairs > 1:
        gen[1] += torch.randint(0, 2, (3, H, W), generator=g, dtype=torch.int16) * 2 - 1
    if pairs > 2:
        gen[2:] += torch.randint(-40, 41, (pairs - 2, 3, H, W), generator=g, dtype=torch.int16)
    return gt.to(torch.uint8), gen.to(torch.uint8)


def rel_err(v, ref, first=1):
    """Worst |v - ref| / |ref| over the pairs first.. (pair 0 of make_pairs is the identical one)."""
    v, ref = torch.as_tensor(v, dtype=torch.float64)[first:], torch.as_tensor(ref, dtype=torch.float64)[first:]
    return float(((v - ref).abs() / ref.abs()).max())
