"""ctrlv_frame_stats, ctrlv_frame_ssim and ctrlv_resize_frames_u8 on the device (include/ctrlv_hip.h; csrc/frame_quality.hip,
csrc/pipeline_io.hip) against the float64 restatement of tests/frame_quality_ref.py (pinned by tests/test_frame_quality_cpu.py)
and against PIL: exact integers, SSIM within 2e-5 on every case -- the constant-250 pair that plain fp32 loses by itself --, bit
equality run to run, across batch sizes and pointer alignments, a differing pixel walked across the tile seams, guard bands
around every output and workspace, R = 0, the refusals, the three PIL filters byte for byte, and the whole metric end to end
through metrics.frame_quality and through raw ctypes."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import frame_quality_ref as Q
from tests import guarded as Gd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["x".join(map(str, s)) for s in Q.SHAPES]


ALL_KINDS = [(1, len(Q.KINDS), 11, 11), (1, len(Q.KINDS), 12, 75)]        # every kind of pair at the two smallest sizes


def _start(shape):
    """Where a shape's frames start in the cycle of kinds: the shapes of the list start one kind apart, so that the one- and
    two-frame shapes see different kinds."""
    return Q.SHAPES.index(shape) if shape in Q.SHAPES else 0


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(gt, gen, ssim, stats) of a shape, all on the host: computed once, shared, never modified."""
    gt, gen = Q.clips(shape, _start(shape))
    for a in (gt, gen):
        a.setflags(write=False)
    return gt, gen, Q.ssim_clip(gt, gen), Q.stats_clip(gt, gen)


def _unaligned(t):
    """The same bytes one byte off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 32, dtype=torch.uint8, device=t.device)
    off = (-buf.data_ptr()) % 16 + 1
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 1 and out.is_contiguous()
    return out


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _outside_unchanged(before, buf, flat, what):
    changed = Gd.as_int(buf) != Gd.as_int(before)
    lo = flat.storage_offset() - buf.storage_offset()
    changed.view(-1)[lo:lo + flat.numel()] = False
    assert not bool(changed.any()), f"{what}: written outside"


@pytest.mark.parametrize("shape", Q.SHAPES, ids=IDS)
def test_stats_are_exact_aligned_and_unaligned(hip_lib, shape):
    from ctrlv_amd import ops
    n, F, H, W = shape
    gt, gen, _, want = _case(shape)
    d_gt, d_gen = _dev(gt), _dev(gen)
    nbytes = n * F * 3 * 8
    for a, b in ((d_gt, d_gen), (_unaligned(d_gt), _unaligned(d_gen))):
        buf, flat = Gd.guarded_flat(nbytes, torch.uint8, DEV)
        before = buf.clone()
        out = flat.view(torch.int64).view(n, F, 3)
        got = ops.frame_stats(a, b, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want), (shape, got.cpu().tolist(), want.tolist())
        Gd.check_written_only_inside(before, buf, flat.view(1, nbytes), torch.from_numpy(want).view(torch.uint8).view(1, nbytes),
                                     what=f"stats {shape}")


@pytest.mark.parametrize("shape", Q.SHAPES + ALL_KINDS, ids=IDS + ["x".join(map(str, s)) for s in ALL_KINDS])
def test_ssim_is_the_restatement_bit_stable_and_writes_nowhere_else(hip_lib, shape):
    from ctrlv_amd import _lib, ops
    n, F, H, W = shape
    gt, gen, want, _ = _case(shape)
    kinds = Q.clip_kinds(shape, _start(shape))
    d_gt, d_gen = _dev(gt), _dev(gen)
    need = _lib.load().ctrlv_frame_ssim_ws_bytes(n, F, H, W)
    assert need > 0 and need % 8 == 0
    # tests/guarded.py has no fill pattern for float64: the doubles are guarded as pairs of fp32 sentinel NaNs
    obuf, oflat = Gd.guarded_flat(2 * n * F, torch.float32, DEV)
    wbuf, wflat = Gd.guarded_flat(need, torch.uint8, DEV)
    assert oflat.data_ptr() % 8 == 0 and wflat.data_ptr() % 8 == 0
    o0, w0 = obuf.clone(), wbuf.clone()
    out = oflat.view(torch.float64).view(n, F)
    got = ops.frame_ssim(d_gt, d_gen, out=out, workspace=wflat)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    _outside_unchanged(o0, obuf, oflat, f"ssim {shape}")
    _outside_unchanged(w0, wbuf, wflat, f"ssim workspace {shape}")
    # every output element was written: none still holds the sentinel's bits (a NaN result -- R = 0 -- has other bits)
    sentinel = Gd.fill_bits(torch.float32, "sentinel")
    assert not bool((Gd.as_int(oflat) == sentinel).any()), "an ssim element was not written"
    unwritten = int.from_bytes(bytes([Gd.fill_bits(torch.uint8, "sentinel")]) * 8, "little", signed=True)
    assert not bool((wflat.view(torch.int64) == unwritten).any()), "a workspace slot was not written"
    vals = got.cpu().numpy()
    err = np.abs(vals - want)
    print(f"ssim {shape}: worst |device - restatement| = {err.max():.3e}", {k: float(e) for k, e in zip(sum(kinds, []), err.ravel())})
    assert np.all(err <= Q.BOUND), (shape, err.tolist(), vals.tolist(), want.tolist())
    for i in range(n):
        for f in range(F):
            if kinds[i][f] == "same":
                assert vals[i, f] == 1.0, (shape, i, f, vals[i, f])
            if kinds[i][f] == "flat250":               # the pair plain fp32 arithmetic about 127.5 loses (1e-3 and more)
                assert abs(vals[i, f] - want[i, f]) <= Q.BOUND, ("the constant-250 pair", shape, vals[i, f], want[i, f])
    # run to run, unaligned inputs, a clip alone
    again = ops.frame_ssim(d_gt, d_gen)
    assert torch.equal(again, got)
    shifted = ops.frame_ssim(_unaligned(d_gt), _unaligned(d_gen))
    assert torch.equal(shifted, got)
    if n > 1:
        alone = ops.frame_ssim(d_gt[1:2].contiguous(), d_gen[1:2].contiguous())
        assert torch.equal(alone[0], got[1])


def test_the_constant_250_pair_at_12_x_75(hip_lib):
    """The case that fails without the pilot: 250 everywhere, one pixel at 247; R = 3 and C2 = 0.0081."""
    from ctrlv_amd import ops
    gt, gen = Q.pair("flat250", 12, 75, 1)
    want = Q.ssim_u8(gt, gen)
    got = float(ops.frame_ssim(_dev(gt[None, None]), _dev(gen[None, None]))[0, 0])
    print(f"constant-250 pair: device {got!r}, restatement {want!r}, difference {abs(got - want):.3e}")
    assert abs(got - want) <= Q.BOUND, (got, want)


def test_a_differing_pixel_across_the_tile_seams(hip_lib):
    """12 x 75: 65 output columns, so two 64-column tiles; the pixel's 11-column footprint crosses the seam (output columns 63 | 64,
    image columns 68 | 69) for the pixel columns 58 .. 74.  Every column is visited, one frame per column in one batch."""
    from ctrlv_amd import ops
    H, W = 12, 75
    base, _ = Q.pair("noise", H, W, 21)
    gt = np.repeat(base[None], W, axis=0)
    gen = gt.copy()
    for x in range(W):
        gen[x, :, 6, x] = gen[x, :, 6, x] ^ 0x40
    want = np.array([Q.ssim_u8(gt[x], gen[x]) for x in range(W)])
    got = ops.frame_ssim(_dev(gt[None]), _dev(gen[None])).cpu().numpy()[0]
    err = np.abs(got - want)
    print(f"seams: worst {err.max():.3e} at column {int(err.argmax())}")
    assert np.all(err <= Q.BOUND), err.tolist()
    assert len(set(np.round(want, 12))) > W // 2          # the pixel's place matters: the cases are not one case


def test_a_constant_pair_inside_a_batch_is_nan_and_disturbs_nothing(hip_lib):
    from ctrlv_amd import metrics, ops
    shape = (1, 3, 37, 70)
    gt, gen = (a.copy() for a in Q.clips(shape, start=1))
    gt[0, 1], gen[0, 1] = 9, 9
    want_s, want_p = Q.ssim_clip(gt, gen), Q.psnr_clip(gt, gen)
    d_gt, d_gen = _dev(gt), _dev(gen)
    st = ops.frame_stats(d_gt, d_gen)
    assert st[0, 1].tolist() == [9, 9, 0]
    got = ops.frame_ssim(d_gt, d_gen, st).cpu().numpy()
    assert math.isnan(got[0, 1]) and math.isnan(want_s[0, 1])
    assert np.all(np.abs(got[0, [0, 2]] - want_s[0, [0, 2]]) <= Q.BOUND)
    q = metrics.frame_quality(d_gt, d_gen)
    assert q["ssim"].shape == q["psnr"].shape == (1, 3) and q["ssim"].dtype == q["psnr"].dtype == np.float64
    assert math.isnan(q["ssim"][0, 1]) and math.isnan(q["psnr"][0, 1])
    assert np.array_equal(q["ssim"][0, [0, 2]], got[0, [0, 2]])
    assert q["psnr"][0, [0, 2]] == pytest.approx(want_p[0, [0, 2]], rel=1e-9)
    one = metrics.frame_quality(d_gt[0], d_gen[0])
    assert one["ssim"].shape == (3,) and np.array_equal(one["ssim"][[0, 2]], got[0, [0, 2]])


def test_refusals_name_the_entry_point_and_launch_nothing(hip_lib):
    from ctrlv_amd import _lib
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, F, H, W = 1, 2, 12, 75
    gt = torch.zeros(n, F, 3, H, W, dtype=torch.uint8, device=DEV)
    stats = torch.full((n * F * 3 + 1,), -7, dtype=torch.int64, device=DEV)
    ssim = torch.full((n * F,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((lib.ctrlv_frame_ssim_ws_bytes(n, F, H, W),), 0x5A, dtype=torch.uint8, device=DEV)
    dst = torch.full((6, 5, 7), 0x5A, dtype=torch.uint8, device=DEV)
    rws = torch.full((lib.ctrlv_resize_frames_ws_bytes(6, H, W, 5, 7, 3),), 0x5A, dtype=torch.uint8, device=DEV)
    g, s, o, w = gt.data_ptr(), stats.data_ptr(), ssim.data_ptr(), ws.data_ptr()

    def refused(rc, code, *words):
        msg = _lib.last_error(lib)
        assert rc == code, (rc, code, msg)
        for word in words:
            assert word in msg, (word, msg)

    refused(lib.ctrlv_frame_ssim(g, g, n, F, 10, W, s, o, w, ws.numel(), st), -2, "frame_ssim", "10")              # H = 10
    refused(lib.ctrlv_frame_ssim(g, g, n, F, H, 10, s, o, w, ws.numel(), st), -2, "frame_ssim")
    assert lib.ctrlv_frame_ssim_ws_bytes(n, F, 10, W) == 0
    refused(lib.ctrlv_frame_ssim(g, None, n, F, H, W, s, o, w, ws.numel(), st), -1, "frame_ssim", "null")          # a null pointer
    refused(lib.ctrlv_frame_ssim(g, g, n, F, H, W, s + 4, o, w, ws.numel(), st), -1, "frame_ssim", "stats")        # misaligned
    refused(lib.ctrlv_frame_ssim(g, g, n, F, H, W, s, o, w, ws.numel() - 1, st), -5, "frame_ssim", "ws_bytes")     # short
    refused(lib.ctrlv_frame_ssim(g, g, 1 << 20, 1 << 10, 64, 1 << 14, s, o, w, ws.numel(), st), -2, "frame_ssim", "workgroups")
    refused(lib.ctrlv_frame_stats(g, None, n, F, H, W, s, st), -1, "frame_stats", "null")
    refused(lib.ctrlv_frame_stats(g, g, n, F, H, W, s + 4, st), -1, "frame_stats", "stats")
    refused(lib.ctrlv_frame_stats(g, g, n, 0, H, W, s, st), -2, "frame_stats")
    refused(lib.ctrlv_resize_frames_u8(g, 6, H, W, dst.data_ptr(), 5, 7, 0, rws.data_ptr(), rws.numel(), st), -1,  # NEAREST
            "resize_frames", "filter")
    refused(lib.ctrlv_resize_frames_u8(g, 6, H, W, dst.data_ptr(), 5, 7, 4, rws.data_ptr(), rws.numel(), st), -1,
            "resize_frames", "filter")
    assert lib.ctrlv_resize_frames_ws_bytes(6, H, W, 5, 7, 4) == 0
    refused(lib.ctrlv_resize_frames_u8(g, 6, 170, W, dst.data_ptr(), 10, 7, 3, rws.data_ptr(), rws.numel(), st), -2,
            "resize_frames", "down-scale")                                                                         # above 16 x
    refused(lib.ctrlv_resize_frames_u8(g, 6, H, W, dst.data_ptr(), 5, 7, 3, rws.data_ptr(), rws.numel() - 1, st), -5,
            "resize_frames", "ws_bytes")
    refused(lib.ctrlv_resize_frames_u8(g, 6, H, W, None, 5, 7, 3, rws.data_ptr(), rws.numel(), st), -1, "resize_frames", "null")
    torch.cuda.synchronize()
    assert bool((stats == -7).all()) and bool((ssim == -7.0).all())                # nothing was launched
    assert bool((ws == 0x5A).all()) and bool((dst == 0x5A).all()) and bool((rws == 0x5A).all())
    from ctrlv_amd import ops
    with pytest.raises(ValueError, match="frame_ssim"):
        ops.frame_ssim(gt[..., :10, :].contiguous(), gt[..., :10, :].contiguous())
    with pytest.raises(ValueError, match="resize_frames"):
        ops.resize_frames_u8(gt, 5, 7, resample=0)
    with pytest.raises(ValueError, match="resample"):
        ops.resize_frames_u8(gt, 5, 7, resample="nearest")


RESIZES = [((37, 70), (23, 41), 4), ((20, 30), (64, 100), 4), ((64, 129), (64, 41), 4), ((320, 512), (256, 410), 3)]


@pytest.mark.parametrize("src,dst,planes", RESIZES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d, _ in RESIZES])
@pytest.mark.parametrize("resample", ["bicubic", "bilinear", "lanczos"])
def test_resize_is_pil_byte_for_byte_and_writes_nowhere_else(hip_lib, resample, src, dst, planes):
    from PIL import Image
    from ctrlv_amd import _lib, ops
    code = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "lanczos": Image.LANCZOS}[resample]
    assert int(code) == ops.RESAMPLE[resample]
    rng = np.random.default_rng(src[1] * 3 + dst[0])
    img = rng.integers(0, 256, size=(planes, src[0], src[1]), dtype=np.uint8)
    img[:, :4, :4], img[:, -4:, -4:], img[:, :4, -4:] = 255, 0, 255            # saturated corners: the clip8 of the overshoot
    want = torch.from_numpy(np.stack([np.asarray(Image.fromarray(p).resize((dst[1], dst[0]), resample=code)) for p in img]))
    x = _dev(img)
    got = ops.resize_frames_u8(x, *dst, resample=resample)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    # ... and PIL's resize of the RGB image of three stacked planes is the planar result
    rgb = np.asarray(Image.fromarray(np.ascontiguousarray(img[:3].transpose(1, 2, 0))).resize((dst[1], dst[0]), resample=code))
    assert torch.equal(got[:3].cpu(), torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))))
    # guard bands around the output and the workspace, leading dimensions kept
    need = _lib.load().ctrlv_resize_frames_ws_bytes(planes, src[0], src[1], dst[0], dst[1], int(code))
    obuf, oflat = Gd.guarded_flat(want.numel(), torch.uint8, DEV)
    wbuf, wflat = Gd.guarded_flat(need, torch.uint8, DEV)
    assert wflat.data_ptr() % 16 == 0
    o0, w0 = obuf.clone(), wbuf.clone()
    ops.resize_frames_u8(x.view(1, planes, *src), *dst, resample=int(code), out=oflat.view(1, planes, *dst), workspace=wflat)
    torch.cuda.synchronize()
    Gd.check_written_only_inside(o0, obuf, oflat.view(1, -1), expected=want.view(1, -1), what="resize_frames_u8 dst")
    _outside_unchanged(w0, wbuf, wflat, "resize_frames_u8 workspace")
    assert torch.equal(oflat.view(want.shape).cpu(), want)


def test_frame_quality_end_to_end_and_from_a_foreign_host(hip_lib):
    """metrics.frame_quality(size=(256, 410)) on (1, 2, 3, 320, 512) against the restatement applied to PIL's bicubic frames; then
    the same three calls through raw ctypes on one stream with no synchronisation in between."""
    from PIL import Image
    from ctrlv_amd import _lib, metrics
    n, F, H, W, h, w = 1, 2, 320, 512, 256, 410
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:H, 0:W]
    scene = np.stack([(yy + xx) % 256, (3 * yy + xx // 2) % 256, ((yy // 16 + xx // 16) % 2) * 200 + 20]).astype(np.int64)
    gt = np.clip(scene[None, None] + rng.integers(-20, 21, size=(n, F, 3, H, W)), 0, 255).astype(np.uint8)
    gen = np.clip(gt.astype(np.int64) + rng.integers(-12, 13, size=gt.shape), 0, 255).astype(np.uint8)
    gen[0, 1] = np.roll(gt[0, 1], 3, axis=-1)

    def pil(a):
        return np.stack([np.stack([np.asarray(Image.fromarray(p).resize((w, h), resample=Image.BICUBIC)) for p in fr]) for fr in a[0]])[None]
    r_gt, r_gen = pil(gt), pil(gen)
    want_s, want_p = Q.ssim_clip(r_gt, r_gen), Q.psnr_clip(r_gt, r_gen)
    d_gt, d_gen = _dev(gt), _dev(gen)
    q = metrics.frame_quality(d_gt, d_gen, size=(h, w))
    print("end to end: ssim", q["ssim"].tolist(), want_s.tolist(), "psnr", q["psnr"].tolist(), want_p.tolist())
    assert q["ssim"].shape == (n, F) and q["psnr"].shape == (n, F)
    assert q["psnr"] == pytest.approx(want_p, rel=1e-9)
    assert np.all(np.abs(q["ssim"] - want_s) <= Q.BOUND), (q["ssim"].tolist(), want_s.tolist())
    summary = metrics.quality_summary(q["ssim"], q["psnr"])
    assert summary["ssim_score_image"] == pytest.approx(Q.quality_summary(want_s, want_p)[0], abs=Q.BOUND)

    # ---- a foreign host: raw pointers, one stream, no synchronisation between the calls
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    planes = n * F * 3
    rs_bytes = lib.ctrlv_resize_frames_ws_bytes(planes, H, W, h, w, 3)
    ss_bytes = lib.ctrlv_frame_ssim_ws_bytes(n, F, h, w)
    assert rs_bytes > 0 and ss_bytes > 0
    rws = torch.empty(rs_bytes, dtype=torch.uint8, device=DEV)
    sws = torch.empty(ss_bytes, dtype=torch.uint8, device=DEV)
    s_gt = torch.empty(n, F, 3, h, w, dtype=torch.uint8, device=DEV)
    s_gen = torch.empty_like(s_gt)
    stats = torch.empty(n, F, 3, dtype=torch.int64, device=DEV)
    ssim = torch.empty(n, F, dtype=torch.float64, device=DEV)
    for src, dst in ((d_gt, s_gt), (d_gen, s_gen)):
        rc = lib.ctrlv_resize_frames_u8(src.data_ptr(), planes, H, W, dst.data_ptr(), h, w, 3, rws.data_ptr(), rs_bytes, st)
        assert rc == 0, _lib.last_error(lib)
    rc = lib.ctrlv_frame_stats(s_gt.data_ptr(), s_gen.data_ptr(), n, F, h, w, stats.data_ptr(), st)
    assert rc == 0, _lib.last_error(lib)
    rc = lib.ctrlv_frame_ssim(s_gt.data_ptr(), s_gen.data_ptr(), n, F, h, w, stats.data_ptr(), ssim.data_ptr(), sws.data_ptr(),
                              ss_bytes, st)
    assert rc == 0, _lib.last_error(lib)
    torch.cuda.synchronize()
    assert torch.equal(s_gt.cpu(), torch.from_numpy(r_gt)) and torch.equal(s_gen.cpu(), torch.from_numpy(r_gen))
    assert np.array_equal(stats.cpu().numpy(), Q.stats_clip(r_gt, r_gen))
    assert np.array_equal(ssim.cpu().numpy(), q["ssim"])
    psnr = [[metrics.psnr_from_stats(*row, 3 * h * w) for row in clip] for clip in stats.cpu().tolist()]
    assert np.array_equal(np.array(psnr), q["psnr"])
