"""Box frames from coordinates on the device (include/ctrlv_hip.h: ctrlv_render_box_frames, ctrlv_box_frames_cond,
ctrlv_pipeline_generate_from_boxes; csrc/box_render.hip), byte for byte against the numpy restatement of the header's integer
picture (tests/box_render_ref.py, proven in tests/test_box_render_cpu.py).  The shapes are the smallest at which the kernel can go
wrong: a 128 x 32 tile means 37 x 53 has a partial tile, two tile rows and a tail in x; 40 x 150 adds a tile edge in x and rows
whose start is not 4-byte aligned.  The driver and the compositions run on the tiny plans of tests/test_pipeline_plan_gpu.py and
tests/test_train_batch_plan_gpu.py, reused by import."""
import contextlib
import ctypes
import gc

import numpy as np
import pytest
import torch

from tests import box_render_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 2 ** 31 - 1


def upload(objects, frames, n_clips=None, num_frames=None):
    from ctrlv_amd.boxes import BoxTable
    n = 1 if n_clips is None else n_clips
    return BoxTable.from_records(objects, frames, n, len(frames) // n if num_frames is None else num_frames).to(DEV)


def render(objects, frames, Hs, Ws, **kw):
    """The kernel's frames (n_frames, 3, Hs, Ws) inside guard bands at an odd offset, which must survive."""
    from ctrlv_amd import ops
    t = upload(objects, frames, **kw)
    n, pad = len(frames) * 3 * Hs * Ws, 4099
    buf = torch.full((n + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
    out = ops.render_box_frames(t, (Hs, Ws), out=buf[pad:pad + n].view(t.n_clips, t.num_frames, 3, Hs, Ws))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), "a write outside the frames"
    return out.reshape(len(frames), 3, Hs, Ws).cpu().numpy()


def check(objects, frames, Hs, Ws, **kw):
    want = B.render(objects, frames, Hs, Ws)
    got = render(objects, frames, Hs, Ws, **kw)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [(int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:5]])
    return want


def placement(Hs, Ws):
    """FILL | OUTLINE boxes: across the tile edges (y = 32, x = 128), on the border, partly and wholly outside, reversed, degenerate,
    and with coordinates beyond the +-8191 clamp."""
    boxes = [(5, 28, 20, 36), (Ws - 30, 30, Ws - 3, 33), (118, 10, 135, 20), (127, 2, 128, 6), (0, 0, 9, 7), (Ws - 1, Hs - 1, Ws - 6, Hs - 5),
             (-5, -4, 8, 8), (-50, -50, -20, -20), (Ws + 3, 5, Ws + 40, 9), (-1, 12, 0, 14), (30, 15, 30, 15), (33, 2, 33, 25),
             (-100000, 20, 100000, 22), (40, -BIG, 43, BIG), (BIG, BIG, BIG - 5, BIG - 5), (24, 33, 47, 34)]
    return [B.obj(*b, fill=(60 + 11 * i, 250 - 9 * i, 51 + 5 * i), line=(255 - 7 * i, 40 + 3 * i, 128), flags=B.FILL | B.OUTLINE)
            for i, b in enumerate(boxes)]


def wires(Hs, Ws):
    """WIRE objects whose fourteen edges are horizontal, vertical, 45 degrees, steep, shallow, of zero length, across the tile
    edges, and partly far outside (corners beyond the clamp)."""
    sets = [
        [(5, 5), (5, 5), (10, 5), (30, 5), (10, 25), (30, 25), (5, 35), (25, 35)],           # zero-length 0-1, horizontals, verticals
        [(2, 2), (20, 20), (40, 3), (45, 36), (12, 30), (50, 31), (0, 36), (36, 0)],          # 45 degrees, steep, shallow
        [(Ws - 1, 0), (Ws - 1, Hs - 1), (0, Hs - 1), (0, 0), (Ws // 2, -9), (Ws // 2, Hs + 9), (-9, Hs // 2), (Ws + 9, Hs // 2)],
        [(30000, 30000), (-30000, -30000), (26, 17), (-32768, 17), (26, 32767), (27, 18), (32767, -32768), (20, 20)],
        [(120, 30), (135, 34), (126, 29), (130, 35), (110, 33), (140, 31), (128, 0), (128, 39)],    # around (128, 32)
    ]
    return [B.obj(corner=c, line=(40 + 50 * i, 255 - 60 * i, 10 + 30 * i), flags=B.WIRE) for i, c in enumerate(sets)]


SIZES = [(37, 53), (40, 150)]


@pytest.mark.parametrize("size", SIZES, ids=["37x53", "40x150"])
def test_geometry_and_placement(hip_lib, size):
    Hs, Ws = size
    p, w = placement(Hs, Ws), wires(Hs, Ws)
    objects, frames = B.tables([p, w, [o for pair in zip(p, w) for o in pair], [p[12]]])
    want = check(objects, frames, Hs, Ws)
    assert all(want[j].any() for j in range(len(frames)))
    assert want[0][:, 21, :].all() and want[3][:, 21, 0].all()          # the row clamped from +-100000 spans the image


def test_every_single_object_alone(hip_lib):
    """One object per frame: a wrong primitive shows up by itself, not under a later object."""
    Hs, Ws = 40, 150
    objs = placement(Hs, Ws) + wires(Hs, Ws)
    for o in wires(Hs, Ws):
        thin = o.copy()
        thin["flags"] = B.WIRE | B.FILL | B.OUTLINE
        thin["x1"], thin["y1"], thin["x2"], thin["y2"] = 100, 3, 140, 38
        thin["fill_rgb"][:3] = (77, 0, 201)
        objs.append(thin)
    objects, frames = B.tables([[o] for o in objs])
    check(objects, frames, Hs, Ws)


def test_painters_order_and_the_per_channel_masks(hip_lib):
    Hs, Ws = 37, 53
    a = B.obj(4, 4, 30, 30, fill=(200, 0, 90), line=(0, 255, 31), corner=[(2, 2), (34, 33), (2, 33), (34, 2), (10, 8), (40, 9), (8, 30), (45, 28)],
              flags=B.FILL | B.OUTLINE | B.WIRE)
    b = B.obj(12, 1, 40, 20, fill=(0, 93, 0), line=(255, 0, 0), corner=[(1, 1), (50, 35), (50, 1), (1, 35), (20, 0), (20, 36), (0, 18), (52, 18)],
              flags=B.FILL | B.OUTLINE | B.WIRE)
    c = B.obj(20, 10, 50, 36, fill=(51, 51, 0), line=(0, 0, 254), corner=[(25, 5), (25, 30), (30, 5), (31, 31), (5, 15), (48, 16), (6, 22), (47, 21)],
              flags=B.FILL | B.OUTLINE | B.WIRE)
    orders = [[a, b, c], [c, b, a], [b, a, c], [a], [a, a]]
    objects, frames = B.tables(orders)
    want = check(objects, frames, Hs, Ws)
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2])      # the order matters in this scene
    assert np.array_equal(want[3], want[4])
    # a zero component lets the layer below show through in that channel only: somewhere T's red is 0 under b and U's is not
    both = (want[0] != 0).sum(axis=0)
    assert set(np.unique(both)) >= {0, 1, 2, 3}


@pytest.mark.parametrize("count", [70, 300], ids=["70_crosses_a_wave", "300_crosses_a_round"])
def test_many_objects_on_one_tile_keep_their_order(hip_lib, count):
    """Every object covers the first tile (and misses the second tile row or not, by turns), so the compaction's slots cross a
    64-object ballot and, at 300, a 256-object round; culled objects in between shift the survivors' slots."""
    Hs, Ws = 37, 53
    rng = np.random.RandomState(count)
    objs = []
    for i in range(count):
        x1, y1 = rng.randint(0, 20), rng.randint(0, 14)
        x2, y2 = rng.randint(30, Ws), rng.randint(16, Hs if i % 3 else 31)
        col = tuple(int(v) for v in rng.randint(0, 256, 3))
        flags = (B.FILL, B.OUTLINE, B.FILL | B.OUTLINE, B.WIRE)[i % 4]
        corner = [(int(rng.randint(-5, Ws + 5)), int(rng.randint(-5, Hs + 5))) for _ in range(8)]
        objs.append(B.obj(x1, y1, x2, y2, fill=col, line=col[::-1], corner=corner, flags=flags))
    # culled ones in between shift the survivors' slots
    for i in range(0, count, 7):
        objs[i] = B.obj(-40, -40, -20, -20, fill=(1, 2, 3), line=(4, 5, 6), flags=B.FILL | B.OUTLINE)
    objects, frames = B.tables([objs, objs[::-1]])
    want = check(objects, frames, Hs, Ws)
    assert not np.array_equal(want[0], want[1])


def scene(n, F, Hs, Ws, seed=0):
    """n clips x F frames with different counts; frame 1 of clip 0 has none; the last frame of every clip is a trajectory frame
    with overlapping discs."""
    rng = np.random.RandomState(seed)
    per_frame, kinds = [], []
    for ci in range(n):
        for fi in range(F):
            k = 0 if (ci, fi) == (0, 1) else 2 + (3 * ci + 2 * fi) % 5
            objs = []
            for j in range(k):
                x1, x2 = sorted(int(v) for v in rng.randint(-6, Ws + 6, 2))
                y1, y2 = sorted(int(v) for v in rng.randint(-6, Hs + 6, 2))
                cam = (ci + j) % 2
                corner = [(int(rng.randint(-8, Ws + 8)), int(rng.randint(-8, Hs + 8))) for _ in range(8)]
                if fi == F - 1:
                    corner[0] = (12 + 5 * j, 12 + 3 * j)                  # 5 apart, radius 20: they overlap
                objs.append(B.obj(x1, y1, x2, y2, fill=tuple(int(v) for v in rng.randint(50, 255, 3)), line=B.PALETTE[(ci + fi + j) % 11],
                                  corner=corner, flags=B.FILL | (B.WIRE if cam else B.OUTLINE)))
            per_frame.append(objs)
            kinds.append(1 if fi == F - 1 else 0)
    return B.tables(per_frame, kinds)


def test_the_frame_table(hip_lib):
    Hs, Ws, n, F = 37, 53, 2, 3
    objects, frames = scene(n, F, Hs, Ws)
    want = check(objects, frames, Hs, Ws, n_clips=n, num_frames=F)
    assert not want[1].any() and all(want[j].any() for j in (0, 2, 3, 4, 5))
    # a trajectory frame: the inner disc's colour at its centre, the outer disc's colour between the radii, in table order
    last = objects[int(frames[2]["first"]) + int(frames[2]["count"]) - 1]
    cx, cy = (int(v) for v in last["corner"][0])
    assert tuple(want[2][:, cy, cx]) == tuple(last["line_rgb"][:3]) and tuple(want[2][:, cy, cx + 15]) == tuple(last["fill_rgb"][:3])
    # first / count out of range: that frame is empty (or cut to the table), its neighbours are untouched
    nobj = len(objects)
    for first, count in ((-1, 3), (nobj, 1), (BIG, 1), (-BIG - 1, BIG), (0, -5), (0, 0), (nobj - 1, BIG), (2, BIG), (nobj - 2, 50)):
        fr = frames.copy()
        fr[3]["first"], fr[3]["count"] = first, count
        got = check(objects, fr, Hs, Ws, n_clips=n, num_frames=F)
        for j in (0, 1, 2, 4, 5):
            assert np.array_equal(got[j], want[j])
        if first < 0 or first >= nobj or count <= 0:
            assert not got[3].any()
        else:
            assert got[3].any()


def test_a_clip_alone_is_the_clip_in_the_batch_and_runs_repeat(hip_lib):
    Hs, Ws, n, F = 37, 53, 2, 3
    objects, frames = scene(n, F, Hs, Ws, seed=3)
    batch = render(objects, frames, Hs, Ws, n_clips=n, num_frames=F)
    again = render(objects, frames, Hs, Ws, n_clips=n, num_frames=F)
    assert np.array_equal(batch, again)
    for ci in range(n):
        alone = render(objects, frames[ci * F:(ci + 1) * F], Hs, Ws)
        assert np.array_equal(alone, batch[ci * F:(ci + 1) * F])
    # through the Python table: BoxTable.clip
    from ctrlv_amd import ops
    t = upload(objects, frames, n_clips=n, num_frames=F)
    one = ops.render_box_frames(t.clip(1), (Hs, Ws))
    assert one.shape == (1, F, 3, Hs, Ws) and np.array_equal(one[0].cpu().numpy(), batch[F:])


def test_an_object_limit_of_1024_per_frame(hip_lib):
    Hs, Ws = 8, 8
    objs = [B.obj(i % 8, (i // 8) % 8, i % 8, (i // 8) % 8, fill=(50 + i % 200, 60, 70 + i // 8), flags=B.FILL) for i in range(1100)]
    objects, frames = B.tables([objs])
    want = check(objects, frames, Hs, Ws)
    cut, _ = B.tables([objs[:1024]])
    assert np.array_equal(want, B.render(cut, frames, Hs, Ws))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("size", [(16, 24), (37, 53)], ids=["to_16x24", "same_size"])
def test_box_frames_cond_is_render_resize_normalize(hip_lib, dtype, size):
    from ctrlv_amd import ops
    Hs, Ws, n, F = 37, 53, 2, 3
    H, W = size
    objects, frames = scene(n, F, Hs, Ws, seed=1)
    t = upload(objects, frames, n_clips=n, num_frames=F)
    u8 = ops.render_box_frames(t, (Hs, Ws))
    assert np.array_equal(u8.cpu().numpy().reshape(n * F, 3, Hs, Ws), B.render(objects, frames, Hs, Ws))
    small = u8 if (H, W) == (Hs, Ws) else ops.resize_frames_u8(u8, H, W, resample="bilinear")
    # ToTensor and Normalize as the data loader runs them, on the CPU: true fp32 divisions, then the cast
    want = small.cpu().float().div(255.0).sub(0.5).div(0.5).to(dtype).to(DEV)
    got, got_u8 = ops.box_frames_cond(t, (Hs, Ws), (H, W), dtype=dtype, return_u8=True)
    plain = ops.box_frames_cond(t, (Hs, Ws), (H, W), dtype=dtype)
    torch.cuda.synchronize()
    assert got.shape == (n, F, 3, H, W) and got.dtype == dtype
    assert torch.equal(got, want) and torch.equal(plain, want) and torch.equal(got_u8, u8)
    assert float(got.float().min()) == -1.0 and float(got.float().max()) > 0.0
    if (H, W) != (Hs, Ws):
        # PIL itself on the rendered frames, for the resize's part of the chain
        from PIL import Image
        rgb = u8[0, 0].permute(1, 2, 0).cpu().numpy()
        pil = np.asarray(Image.fromarray(rgb).resize((W, H), resample=Image.BILINEAR)).transpose(2, 0, 1)
        assert np.array_equal(small[0, 0].cpu().numpy(), pil)


# ------------------------------------------------------------------------------------------------------------------ the driver
@contextlib.contextmanager
def _leaves_no_state_behind():
    """The models and plans below are built for this module alone: torch's global generator is put back as it was found (the
    builders seed it), and what was built is destroyed here -- streams, events and workspaces included -- not whenever a later
    module's allocations happen to start a collection."""
    rng = torch.get_rng_state()
    try:
        yield
    finally:
        torch.set_rng_state(rng)
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.synchronize()


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def setup(request, hip_lib):
    from tests.test_pipeline_plan_gpu import build_setup
    with _leaves_no_state_behind():
        yield build_setup(request.param)


SRC = (97, 150)              # the coordinates' size; the plans work at 128 x 192


def clip_table(n, F, kinds_last=1):
    objects, frames = scene(n, F, *SRC, seed=5)
    if not kinds_last:
        frames["kind"] = 0
    return upload(objects, frames, n_clips=n, num_frames=F)


COMMON = dict(noise_aug_strength=0.02, fps=7, motion_bucket_id=127, min_guidance=1.0, max_guidance=3.0, decode_chunk=2)


@pytest.mark.parametrize("n", [1, 2])
def test_generate_from_boxes_is_the_two_calls_by_hand(setup, n):
    from ctrlv_amd import ops
    from tests.test_pipeline_plan_gpu import F, H, W, same
    s = setup
    t = clip_table(n, F)
    cond = ops.box_frames_cond(t, SRC, (H, W), dtype=s.el)
    want = s.pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, cond=cond, aug_noise=s.aug[:n], conditioning_scale=0.8,
                           **COMMON)
    torch.cuda.synchronize()
    got = s.pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, boxes=t, source_size=SRC, aug_noise=s.aug[:n],
                          conditioning_scale=0.8, **COMMON)
    torch.cuda.synchronize()
    same(got, want)
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0
    # the boxes reach the model: another table, other latents
    other = s.pipe.generate(s.image[:n], s.lat[:n], s.sigmas, s.timesteps, boxes=upload(*scene(n, F, *SRC, seed=6), n_clips=n, num_frames=F),
                            source_size=SRC, aug_noise=s.aug[:n], conditioning_scale=0.8, frames=False, frames_u8=False, **COMMON)
    torch.cuda.synchronize()
    assert not torch.equal(other[0], got[0])


def test_the_from_boxes_workspace_query_refuses_what_the_call_refuses(setup):
    from ctrlv_amd import _lib
    from tests.test_pipeline_plan_gpu import F, H, W
    s = setup
    lib = s.pipe._lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = clip_table(1, F)
    image, lat = s.image[:1].contiguous(), s.lat[:1].contiguous()
    out_lat = torch.full_like(lat, 7.0)
    r, keep = s.pipe.request(image, lat, s.sigmas, s.timesteps, aug_noise=s.aug[:1].contiguous(), conditioning_scale=0.8,
                             out_latents=out_lat, **COMMON)
    b = s.pipe.box_render_request(t, SRC)
    need = lib.ctrlv_pipeline_from_boxes_workspace_bytes(s.pipe._h, ctypes.byref(r), ctypes.byref(b))
    assert need > 0 and need % 256 == 0, _lib.last_error(lib)
    r.cond, r.cond_channels, r.cond_dtype = 0x1000, 3, lib.ctrlv_elem_dtype()
    plain = lib.ctrlv_pipeline_workspace_bytes(s.pipe._h, ctypes.byref(r))
    r.cond = None
    assert need >= plain + F * 3 * H * W * 2
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.ctrlv_pipeline_generate_from_boxes(s.pipe._h, ctypes.byref(r), ctypes.byref(b), ws.data_ptr(), need - 1, st) == -5
    assert str(need) in _lib.last_error(lib) and "ws_bytes" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert bool((out_lat == 7.0).all())                          # nothing was launched
    for field, value, word in (("n_frames", F + 1, "n_frames"), ("src_height", 4097, "source size"), ("src_width", 192 * 17, "down-scale"),
                               ("objects", None, "table is null")):
        bad = s.pipe.box_render_request(t, SRC)
        setattr(bad, field, value)
        assert lib.ctrlv_pipeline_from_boxes_workspace_bytes(s.pipe._h, ctypes.byref(r), ctypes.byref(bad)) == 0
        assert word in _lib.last_error(lib)
        assert lib.ctrlv_pipeline_generate_from_boxes(s.pipe._h, ctypes.byref(r), ctypes.byref(bad), ws.data_ptr(), need, st) < 0
        assert word in _lib.last_error(lib)
    assert lib.ctrlv_pipeline_from_boxes_workspace_bytes(s.pipe_svd._h, ctypes.byref(r), ctypes.byref(b)) == 0
    assert "no ControlNet" in _lib.last_error(lib)
    r.cond = 0x1000
    assert lib.ctrlv_pipeline_from_boxes_workspace_bytes(s.pipe._h, ctypes.byref(r), ctypes.byref(b)) == 0
    assert "cond is set together with boxes" in _lib.last_error(lib)
    r.cond = None
    torch.cuda.synchronize()
    assert bool((out_lat == 7.0).all())
    assert lib.ctrlv_pipeline_generate_from_boxes(s.pipe._h, ctypes.byref(r), ctypes.byref(b), ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert bool((out_lat != 7.0).any())
    del keep


def test_predict_boxes_from_a_table_is_predict_boxes_on_the_rendered_frames(setup):
    """... with the last frame a trajectory frame (the reference's if_last_frame_trajectory at inference)."""
    from ctrlv_amd import ops
    from tests.test_pipeline_plan_gpu import F, H, W, same
    s = setup
    t = clip_table(1, F)
    assert int(t.frames[F - 1, 2]) == 1
    rendered = ops.box_frames_cond(t, SRC, (H, W), dtype=s.el)
    args = (s.image[:1], s.lat[:1], s.sigmas, s.timesteps)
    want = s.pipe_svd.predict_boxes(*args, rendered, 1, aug_noise=s.aug[:1], **COMMON)
    torch.cuda.synchronize()
    got = s.pipe_svd.predict_boxes(*args, num_cond_frames=1, boxes=t, source_size=SRC, aug_noise=s.aug[:1], **COMMON)
    torch.cuda.synchronize()
    same(got, want)
    boxy = s.pipe_svd.predict_boxes(*args, num_cond_frames=1, boxes=clip_table(1, F, kinds_last=0), source_size=SRC, aug_noise=s.aug[:1],
                                    frames=False, frames_u8=False, **COMMON)
    torch.cuda.synchronize()
    assert not torch.equal(boxy[0], got[0])                      # the trajectory frame is another picture


@pytest.mark.parametrize("el", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_training_batch_from_a_table_is_the_batch_from_the_rendered_frames(hip_lib, el):
    from ctrlv_amd import ops
    from ctrlv_amd.training import prepare_batch
    from tests.test_train_batch_plan_gpu import CALL, DP, F, H, K, N, W, bits
    with _leaves_no_state_behind():
        _training_batch_from_a_table(el, ops, prepare_batch, CALL, DP, F, H, K, N, W, bits)


def _train_setup(el, N, F, H, W):
    """The plans and inputs of tests/test_train_batch_plan_gpu.py's setup, built here and dropped after the test (that module keeps
    its own for its whole run)."""
    from ctrlv_amd import DeviceSeed
    from ctrlv_amd.models import AutoencoderKLTemporalDecoder, clip_vision_hip
    from ctrlv_amd.plan import TrainBatchPlan, vae_plan
    from tests import clip_utils as U
    from tests.test_pipeline_plan_gpu import PIPE_CLIP
    from tests.test_train_batch_plan_gpu import CLIP0, SEED, Setup, gen
    s = Setup()
    torch.manual_seed(5)
    s.vae = AutoencoderKLTemporalDecoder().eval().to(DEV, el)
    s.clip = U.build_own(PIPE_CLIP, 31, el, DEV)
    s.plan = TrainBatchPlan(vae_plan(s.vae, dtype=el), clip_vision_hip._plan(s.clip))
    s.seed = DeviceSeed(SEED, clip_index0=CLIP0)
    s.clips = (torch.rand(N, F, 3, H, W, generator=gen(21)) * 2.4 - 1.2).clamp(-1, 1).to(DEV)
    return s


def _training_batch_from_a_table(el, ops, prepare_batch, CALL, DP, F, H, K, N, W, bits):
    s = _train_setup(el, N, F, H, W)
    objects, frames = scene(N, F, *SRC, seed=8)
    frames["kind"] = 0
    t = upload(objects, frames, n_clips=N, num_frames=F)
    rendered = ops.box_frames_cond(t, SRC, (H, W), dtype=el)
    kw = dict(mode="controlnet", seed=s.seed, step=CALL, num_cond_frames=K, dropout_prob=DP, return_noise=True)
    want = s.plan.prepare(s.clips, rendered, **kw)
    got = s.plan.prepare(s.clips, boxes=t, source_size=SRC, **kw)
    batch = prepare_batch(s.plan, s.clips, boxes=t, source_size=SRC, **kw)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want) and "control_cond" in got
    for k in want:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    assert torch.equal(bits(batch["control_cond"]), bits(want["control_cond"]))
    assert float(got["control_cond"].abs().max()) > 0
    with pytest.raises(ValueError, match="mutually exclusive"):
        s.plan.prepare(s.clips, rendered, boxes=t, source_size=SRC, **kw)
    with pytest.raises(ValueError, match="source_size"):
        s.plan.prepare(s.clips, boxes=t, **kw)
