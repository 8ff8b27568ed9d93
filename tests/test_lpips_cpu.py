"""LPIPS without a GPU: the torch restatement (tests/lpips_ref.py), the weight container and its loaders, the split weight
columns against F.unfold, the summary, and what the library decides on the host."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ctrlv_amd.models.lpips_alex import CONVS, LpipsAlexWeights, conv_keys, lin_keys, split_weight_columns
from tests import lpips_ref as R


@pytest.fixture(scope="module")
def weights():
    return LpipsAlexWeights.random(0)


def test_identical_frames_score_exactly_zero_in_every_forward(weights):
    gt, _ = R.make_pairs(37, 50, 2, seed=1)
    for score in (R.forward(weights, gt, gt, torch.float64), R.forward(weights, gt, gt, torch.float32),
                  R.forward_split(weights, gt, gt, torch.bfloat16), R.forward_split(weights, gt, gt, torch.float16)):
        assert score.dtype == torch.float64 and score.tolist() == [0.0, 0.0]


def test_the_split_recovers_what_plain_16_bit_storage_loses(weights):
    """The finding the design rests on, at 37 x 50: on the pair one grey level apart the emulated split forward is within 1e-3 of
    fp64 in both element types and plain bf16 storage is at least 16 times worse than the bf16 split."""
    gt, gen = R.make_pairs(37, 50, 3, seed=2)
    ref = R.forward(weights, gt, gen)
    assert float(ref[0]) == 0.0 and float(ref[1]) > 0.0 and float(ref[2]) > float(ref[1])
    err = {el: abs(float(R.forward_split(weights, gt, gen, el)[1] - ref[1]) / float(ref[1])) for el in (torch.bfloat16, torch.float16)}
    plain = abs(float(R.forward_plain16(weights, gt, gen, torch.bfloat16)[1] - ref[1]) / float(ref[1]))
    print("split bf16 %.3g, split fp16 %.3g, plain bf16 %.3g" % (err[torch.bfloat16], err[torch.float16], plain))
    assert err[torch.bfloat16] < 1e-3 and err[torch.float16] < 1e-3
    assert plain > 16 * err[torch.bfloat16]


def test_random_weights_are_seeded_and_shaped():
    a, b, c = LpipsAlexWeights.random(0), LpipsAlexWeights.random(0), LpipsAlexWeights.random(1)
    assert sorted(a.tensors) == sorted(conv_keys() + lin_keys())
    for l, (i, cin, cout, k, _, _) in enumerate(CONVS):
        w, bias = a.conv(l)
        assert tuple(w.shape) == (cout, cin, k, k) and tuple(bias.shape) == (cout,) and tuple(a.lin(l).shape) == (cout,)
        assert float(a.lin(l).min()) >= 0.0 and float(a.lin(l).max()) <= 2.0 / cout
        assert abs(float(w.std()) / (2.0 / (cin * k * k)) ** 0.5 - 1.0) < 0.1
        assert torch.equal(w, b.conv(l)[0]) and not torch.equal(w, c.conv(l)[0])


def _synthetic_files(weights, tmp_path, ext):
    alex = {k: weights.tensors[k] for k in conv_keys()}
    alex["classifier.1.weight"] = torch.zeros(4, 4)             # torchvision's file has more than the features
    lin = {k: weights.tensors[k] for k in lin_keys()}
    pa, pl = tmp_path / f"alexnet.{ext}", tmp_path / f"alex.{ext}"
    if ext == "safetensors":
        from safetensors.torch import save_file
        save_file(alex, str(pa))
        save_file(lin, str(pl))
    else:
        torch.save(alex, str(pa))
        torch.save(lin, str(pl))
    return alex, lin, pa, pl


@pytest.mark.parametrize("ext", ["pth", "safetensors"])
def test_loaders_map_the_two_published_state_dicts(weights, tmp_path, ext):
    alex, lin, pa, pl = _synthetic_files(weights, tmp_path, ext)
    for got in (LpipsAlexWeights.from_state_dicts(alex, lin), LpipsAlexWeights.from_files(pa, pl)):
        assert sorted(got.tensors) == sorted(conv_keys() + lin_keys())           # classifier.* is dropped
        for k, v in weights.tensors.items():
            assert torch.equal(got.tensors[k], v) and got.tensors[k].dtype == torch.float32
    # a 16-bit file loads as fp32
    half = LpipsAlexWeights.from_state_dicts({k: v.half() for k, v in alex.items()}, lin)
    assert half.conv(0)[0].dtype == torch.float32
    # a missing key is an error that names it, in either dict; so is a wrong shape
    for victim, where in (("features.6.bias", alex), ("lin3.model.1.weight", lin)):
        broken = {k: v for k, v in where.items() if k != victim}
        with pytest.raises(KeyError, match=victim.replace(".", r"\.")):
            LpipsAlexWeights.from_state_dicts(broken if where is alex else alex, broken if where is lin else lin)
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        LpipsAlexWeights.from_state_dicts(dict(alex, **{"features.3.weight": torch.zeros(192, 64, 3, 3)}), lin)


def test_find_looks_under_the_model_root_only(weights, tmp_path, monkeypatch):
    monkeypatch.delenv("CTRLV_MODEL_ROOT", raising=False)
    assert LpipsAlexWeights.find() is None
    monkeypatch.setenv("CTRLV_MODEL_ROOT", str(tmp_path))
    assert LpipsAlexWeights.find() is None                           # the root has no lpips/ directory
    d = tmp_path / "lpips"
    d.mkdir()
    _, _, pa, _ = _synthetic_files(weights, d, "pth")
    found = LpipsAlexWeights.find()
    assert found == (str(pa), str(d / "alex.pth"))
    assert torch.equal(LpipsAlexWeights.from_files(*found).conv(4)[0], weights.conv(4)[0])
    (d / "alex.pth").unlink()
    assert LpipsAlexWeights.find() is None                           # one of the two files alone is nothing


def test_quality_summary_adds_the_plain_mean():
    from ctrlv_amd.metrics import quality_summary
    ssim, psnr = np.array([[0.5, 0.7]]), np.array([[20.0, 30.0]])
    base = quality_summary(ssim, psnr)
    assert "lpips_score" not in base                                 # the default is what it was
    lp = np.array([[0.25, 0.5], [0.0, 0.125]])
    out = quality_summary(ssim, psnr, lpips=lp)
    assert out["lpips_score"] == 0.21875 and {k: out[k] for k in base} == base


@pytest.mark.parametrize("order", [0, 1])
def test_split_weight_columns_match_unfold_on_a_two_channel_toy(order):
    """order 0 is F.unfold's own (c, ky, kx); order 1 is tap-major (ky, kx, c).  A convolution is the unfolded rows against the
    packed columns; the three blocks are whi | wlo | whi and the padding columns are zero."""
    g = torch.Generator().manual_seed(3)
    N, C, k, pad = 5, 2, 3, 1
    w = torch.randn(N, C, k, k, generator=g)
    x = torch.randn(2, C, 4, 6, generator=g)
    K, Kp = C * k * k, 64
    full = split_weight_columns(w, order, torch.float32)
    assert tuple(full.shape) == (N, 3 * Kp)
    cols = full[:, :K]
    assert torch.equal(full[:, 2 * Kp:2 * Kp + K], cols) and not full[:, Kp:2 * Kp].any()      # fp32 "elements": hi = w, lo = 0
    assert not full[:, K:Kp].any() and not full[:, 2 * Kp + K:].any()
    rows = F.unfold(x, k, padding=pad)                                                # (n, C k k, L) in (c, ky, kx) order
    if order == 1:
        rows = rows.reshape(2, C, k * k, -1).permute(0, 2, 1, 3).reshape(2, K, -1)
    y = torch.einsum("nkl,ok->nol", rows.double(), cols.double()).reshape(2, N, 4, 6)
    assert torch.allclose(y, F.conv2d(x.double(), w.double(), None, 1, pad), rtol=0, atol=1e-12)
    # in a 16-bit element type: hi is the rounded weight, hi + lo recovers it to 2^-16 relative
    for el in (torch.bfloat16, torch.float16):
        s = split_weight_columns(w, order, el)
        hi, lo = s[:, :K].float(), s[:, Kp:Kp + K].float()
        assert torch.equal(hi, cols.to(el).float()) and torch.equal(s[:, 2 * Kp:2 * Kp + K].float(), hi)
        assert float(((hi + lo) - cols).abs().max()) <= 2.0 ** -16 * float(cols.abs().max())


def test_library_exports_the_entry_points_and_checks_shapes_on_the_host():
    """Needs no GPU: the plan is created on the host, the geometry is refused before anything touches the device."""
    import __graft_entry__ as g
    g.build()
    assert "lpips.hip" in g.HIP_SOURCES
    from ctrlv_amd import _lib
    for lib in (_lib.load(torch.bfloat16), _lib.load(torch.float16)):
        h = ctypes.c_void_p()
        assert lib.ctrlv_lpips_plan_create(0, ctypes.byref(h)) == 0
        assert lib.ctrlv_lpips_ws_bytes(h, 30, 64, 1) == 0 and "31 x 31" in _lib.last_error(lib)
        assert lib.ctrlv_lpips_ws_bytes(h, 64, 30, 1) == 0
        one, four = lib.ctrlv_lpips_ws_bytes(h, 37, 50, 1), lib.ctrlv_lpips_ws_bytes(h, 37, 50, 4)
        assert 0 < one < four <= 4 * one
        assert lib.ctrlv_lpips_ws_bytes(h, 37, 50, 0) == 0
        with pytest.raises(ValueError, match="not loaded"):
            _lib.check(lib.ctrlv_lpips_frames(h, ctypes.c_void_p(256), ctypes.c_void_p(256), 3, 1, 1, 37, 50, ctypes.c_void_p(256),
                                              ctypes.c_void_p(256), 1 << 30, None), "ctrlv_lpips_frames")
        assert lib.ctrlv_lpips_plan_destroy(h) == 0
        assert [lib.ctrlv_lpips_distance_blocks(p) for p in (1, 64, 65, 88)] == [1, 1, 2, 2]
        with pytest.raises(ValueError, match="k = 3 or 5"):
            _lib.check(lib.ctrlv_lpips_im2col_split(ctypes.c_void_p(256), 1, 0, 1, 3, 5, 64, 64, 7, ctypes.c_void_p(256), None),
                       "ctrlv_lpips_im2col_split")
