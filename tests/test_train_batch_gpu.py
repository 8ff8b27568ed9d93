"""The training-batch kernels on the device (include/ctrlv_hip.h: ctrlv_train_draws, ctrlv_train_assemble,
ctrlv_resize_antialias_clamped; csrc/train_batch.hip) against the numpy restatements of tests/train_batch_ref.py, bit for bit,
in both element builds.  The seed is the one tests/test_train_batch_cpu.py proves to fall into all four dropout regions."""
import numpy as np
import pytest
import torch

from tests import train_batch_ref as T
from tests.test_seeded_gpu import RANDN_ULPS
from tests.test_train_batch_cpu import CALL, CLIP0, CLIPS, DP, SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
# (n, F, L, h, w): plane a multiple of 4 (16-byte path), plane 60 (16-byte path, odd h), and the tail case L = 1, h w = 15
SHAPES = ((2, 3, 4, 4, 4), (2, 4, 4, 3, 5), (2, 3, 1, 3, 5))


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


def gen(seed):
    return torch.Generator().manual_seed(seed)


def name(el):
    return "bf16" if el == torch.bfloat16 else "fp16"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want_np):
    """got: a device tensor (fp32 or an element type); want_np: fp32 numpy holding the exact values."""
    want = np.ascontiguousarray(want_np, dtype=np.float32)
    return np.array_equal(got.detach().float().cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def tables():
    from ctrlv_amd.schedulers import EulerDiscreteScheduler
    s = EulerDiscreteScheduler()
    return s.sigmas[:-1].clone(), s.timesteps.clone()


# ----------------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("size", [1000, 7])
def test_draws_are_the_restatement(el, tables, size):
    from ctrlv_amd import ops
    sig, ts = tables[0][:size].contiguous(), tables[1][:size].contiguous()
    got = ops.train_draws(SEED, CLIPS, sig.to(DEV), ts.to(DEV), clip0=CLIP0, call=CALL, dropout_prob=DP, el=el)
    torch.cuda.synchronize()
    want = T.draws(SEED, CLIPS, sig.numpy(), ts.numpy(), clip0=CLIP0, call=CALL, dropout_prob=DP)
    assert got["indices"].dtype == torch.int32 and np.array_equal(got["indices"].cpu().numpy(), want["indices"])
    for k in ("sigmas", "timesteps", "random_p", "prompt_keep", "image_mask"):
        assert got[k].dtype == torch.float32 and same_bits(got[k], want[k]), k
    # all four regions of p are there (the CPU test's condition, seen on the device's own values)
    keep, image = got["prompt_keep"].cpu(), got["image_mask"].cpu()
    assert {(float(a), float(b)) for a, b in zip(keep, image)} == {(0.0, 1.0), (0.0, 0.0), (1.0, 0.0), (1.0, 1.0)}
    off = ops.train_draws(SEED, CLIPS, sig.to(DEV), ts.to(DEV), clip0=CLIP0, call=CALL, el=el)
    assert float(off["prompt_keep"].min()) == 1.0 and float(off["image_mask"].min()) == 1.0
    assert torch.equal(off["indices"], got["indices"]) and torch.equal(off["random_p"], got["random_p"])


def test_draws_are_keyed_per_clip(el, tables):
    from ctrlv_amd import ops
    sig, ts = tables[0].to(DEV), tables[1].to(DEV)
    a = ops.train_draws(SEED, 3, sig, ts, clip0=5, call=CALL, dropout_prob=DP, el=el)
    b = ops.train_draws(SEED, 1, sig, ts, clip0=6, call=CALL, dropout_prob=DP, el=el)
    c = ops.train_draws(SEED, 3, sig, ts, clip0=5, call=CALL + 1, dropout_prob=DP, el=el)
    for k in a:
        assert torch.equal(a[k][1], b[k][0]), k
    assert not torch.equal(a["random_p"], c["random_p"]) and not torch.equal(a["indices"], c["indices"])


# -------------------------------------------------------------------------------------------------------------------- assembly
def _inputs(shape, seed=1, offset=0):
    """Random fp32 inputs on the device; offset: floats by which every tensor's pointer is moved off its 16-byte alignment."""
    n, F, L, h, w = shape
    g = gen(seed)

    def dev(*s):
        flat = torch.randn(int(np.prod(s)) + offset, generator=g).to(DEV)
        return flat[offset:].view(*s)

    x = dict(target=dev(n, F, L, h, w), noise=dev(n, F, L, h, w), cond_frames=dev(n, F, L, h, w), cond_image=dev(n, L, h, w))
    x["sigmas"] = (torch.rand(n, generator=g) * 20 + 0.01).to(DEV)
    x["image_mask"] = torch.tensor([1.0, 0.0] * n)[:n].to(DEV)
    return x


def _want(x, layout, K, el_name):
    c = {k: v.cpu().numpy() for k, v in x.items()}
    return T.assemble(c["target"], c["noise"], c["sigmas"], c["image_mask"], c["cond_image"], c["cond_frames"], layout, K, el=el_name)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_assembly_with_given_noise_is_the_restatement(el, shape, offset):
    from ctrlv_amd import ops
    F = shape[1]
    x = _inputs(shape, offset=offset)
    assert x["target"].data_ptr() % 16 == (4 * offset) % 16
    for layout, K in ((0, 0), (1, 0), (1, 1), (1, F)):
        for dt, el_name in ((el, name(el)), (torch.float32, None)):
            noisy, sample, _ = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], noise=x["noise"],
                                                  image_mask=x["image_mask"], cond_frames=x["cond_frames"] if layout else None,
                                                  layout=layout, num_cond_frames=K, sample_dtype=dt, el=el)
            torch.cuda.synchronize()
            want_noisy, want_sample = _want(x, layout, K, el_name)
            assert sample.dtype == dt and sample.shape == (shape[0], F, 2 * shape[2]) + shape[3:]
            assert same_bits(noisy, want_noisy), (layout, K)
            assert same_bits(sample, want_sample), (layout, K, dt)
    # without a mask: all ones
    noisy, sample, _ = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], noise=x["noise"], sample_dtype=el)
    y = dict(x, image_mask=torch.ones_like(x["sigmas"]))
    assert same_bits(sample, _want(y, 0, 0, name(el))[1])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_in_kernel_noise_is_randn_then_the_call(el, shape):
    """noise = NULL: the bits of ops.randn(stream 3) followed by the call with that noise, on both access paths; noise_out is
    that noise, within ctrlv_randn's bound of the float64 Box-Muller restatement."""
    from ctrlv_amd import ops
    x = _inputs(shape, seed=2)
    kw = dict(image_mask=x["image_mask"], cond_frames=x["cond_frames"], layout=1, num_cond_frames=1, sample_dtype=el)
    z = ops.randn(SEED, shape, clip0=CLIP0, call=CALL, stream_id=T.STREAM_NOISE, device=DEV)
    want = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], noise=z, **kw)
    got = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], seed=SEED, clip0=CLIP0, call=CALL, return_noise=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    assert torch.equal(bits(got[2]), bits(z))
    ref, r = T.noise(SEED, shape, clip0=CLIP0, call=CALL)
    ulp = np.exp2(np.floor(np.log2(np.maximum(r, 1.0))) - 23)
    err = np.abs(got[2].cpu().numpy().astype(np.float64) - ref) / ulp
    print(f"  noise_out {shape}: largest error {float(err.max()):.3f} ulp of max(r, 1) (bound {RANDN_ULPS})")
    assert float(err.max()) <= RANDN_ULPS
    # the noise did its work: noisy = target + noise * sigma of the restatement on the device's own noise
    c = {k: v.cpu().numpy() for k, v in x.items()}
    assert same_bits(got[0], T.assemble(c["target"], got[2].cpu().numpy(), c["sigmas"], None, c["cond_image"], el=None)[0])


def test_assembly_is_keyed_per_clip_and_blind_to_the_path(el):
    """Clip 1 of a batch at clip0 = 5 is clip 0 of a batch at clip0 = 6; and the element-by-element path (an unaligned target)
    gives the bits of the 16-byte path."""
    from ctrlv_amd import ops
    shape = (3, 3, 4, 4, 4)
    x = _inputs(shape, seed=4)
    kw = dict(layout=1, num_cond_frames=1, sample_dtype=el, seed=SEED, call=CALL, return_noise=True)
    a = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], image_mask=x["image_mask"], cond_frames=x["cond_frames"],
                           clip0=5, **kw)
    b = ops.train_assemble(x["target"][1:2].contiguous(), x["sigmas"][1:2].contiguous(), x["cond_image"][1:2].contiguous(),
                           image_mask=x["image_mask"][1:2].contiguous(), cond_frames=x["cond_frames"][1:2].contiguous(), clip0=6, **kw)
    moved = torch.empty(x["target"].numel() + 1, device=DEV)[1:].view(shape).copy_(x["target"])
    c = ops.train_assemble(moved, x["sigmas"], x["cond_image"], image_mask=x["image_mask"], cond_frames=x["cond_frames"], clip0=5, **kw)
    other = ops.train_assemble(x["target"], x["sigmas"], x["cond_image"], image_mask=x["image_mask"], cond_frames=x["cond_frames"],
                               clip0=5, **dict(kw, call=CALL + 1))
    torch.cuda.synchronize()
    assert moved.data_ptr() % 16 == 4
    for i in range(3):
        assert torch.equal(bits(a[i][1:2]), bits(b[i])), i
        assert torch.equal(bits(a[i]), bits(c[i])), i
    assert not torch.equal(a[2], other[2])


# ------------------------------------------------------------------------------------------------------------- clamped resize
def test_clamped_resize_on_a_step_edge(el):
    """A -1 | +1 step edge, up-scaled (16 x 24 -> 40 x 56): the bicubic overshoots on both sides, so (y + 1) / 2 leaves [0, 1] on
    both.  Against the float64 expression on the unnormalised fp32 output of the same kernel, within the kernel's 2e-5."""
    from ctrlv_amd import ops
    x = torch.ones(2, 3, 16, 24)
    x[:, :, :, :12] = -1.0
    x[1] = x[1].transpose(1, 2).reshape(3, 16, 24)                      # (another pattern: the edge meets the rows at an angle)
    x = x.to(DEV)
    plain = ops.resize_antialias(x, (40, 56))
    got = ops.resize_antialias(x, (40, 56), mean=MEAN, std=STD, clamp=True)
    loose = ops.resize_antialias(x, (40, 56), mean=MEAN, std=STD)
    got_el = ops.resize_antialias(x, (40, 56), mean=MEAN, std=STD, clamp=True, out_dtype=el)
    torch.cuda.synchronize()
    y = plain.cpu().numpy().astype(np.float64)
    u = (y + 1.0) / 2.0
    assert u.min() < -1e-3 and u.max() > 1.0 + 1e-3                     # clamping happens on both sides
    mean, std = np.array(MEAN).reshape(1, 3, 1, 1), np.array(STD).reshape(1, 3, 1, 1)
    want = (np.clip(u, 0.0, 1.0) - mean) / std
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"  clamped resize: {int((u < 0).sum())} values below 0, {int((u > 1).sum())} above 1, max abs error {err:.3e}")
    assert err <= 2e-5
    lo, hi = (np.float32(0) - np.float32(mean)) / np.float32(std), (np.float32(1) - np.float32(mean)) / np.float32(std)
    g32 = got.cpu().numpy()
    assert np.array_equal(g32[u < 0], np.broadcast_to(lo.astype(np.float32), u.shape)[u < 0])
    assert np.array_equal(g32[u > 1], np.broadcast_to(hi.astype(np.float32), u.shape)[u > 1])
    inside = torch.from_numpy((u >= 0) & (u <= 1)).to(DEV)
    assert torch.equal(got[inside], loose[inside]) and not torch.equal(got, loose)
    assert got_el.dtype == el and torch.equal(got_el, got.to(el))


def test_clamped_resize_is_the_plain_one_where_nothing_clamps(el):
    from ctrlv_amd import ops
    x = (torch.rand(2, 3, 61, 90, generator=gen(8)) - 0.5).to(DEV)
    u8 = torch.randint(60, 200, (2, 61, 90, 3), generator=gen(9), dtype=torch.uint8).to(DEV)
    for src in (x, u8):
        for size in ((56, 56), (64, 100)):
            a = ops.resize_antialias(src, size, mean=MEAN, std=STD, clamp=True, out_dtype=el)
            b = ops.resize_antialias(src, size, mean=MEAN, std=STD, out_dtype=el)
            p = ops.resize_antialias(src, size)
            assert float(p.min()) > -1.0 and float(p.max()) < 1.0
            assert torch.equal(bits(a), bits(b)), size
    with pytest.raises(ValueError, match="clamp"):
        ops.resize_antialias(x, (56, 56), clamp=True)
