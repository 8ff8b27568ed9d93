"""Box frames from coordinates, without a GPU: the numpy restatement of include/ctrlv_hip.h's integer picture
(tests/box_render_ref.py) is proven where it can be proven independently -- PIL's filled rectangles, a hand-written ring, the blend
table against float64 --; the library's host helpers (class palette, track colour, corner projection) are held against it through
ctypes; the new entry points refuse by name on the host; and BoxTable.from_labels builds the records it is documented to build.
The picture is this project's stated geometry, not OpenCV's raster (cv2 is not a dependency of the tests)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import box_render_ref as B
from tests.test_box_chain_cpu import _create, _plans
from tests.test_pipeline_plan_cpu import _request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ctrlv_render_box_frames", "ctrlv_box_frames_cond_ws_bytes", "ctrlv_box_frames_cond", "ctrlv_box_class_color",
       "ctrlv_box_track_color", "ctrlv_box_project_corners", "ctrlv_pipeline_from_boxes_workspace_bytes",
       "ctrlv_pipeline_generate_from_boxes")
SCENE = json.load(open(os.path.join(ROOT, "tests", "golden", "box_render_kitti_like.json")))


@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


def grid(H, W):
    return np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")[::-1]


# ---- the restatement itself

BOXES = [(3, 4, 20, 11), (20, 11, 3, 4), (20, 4, 3, 11), (5, 5, 5, 5), (7, 2, 7, 30), (-6, -3, 4, 9), (25, 20, 60, 50), (40, 40, 90, 90),
         (-9, -9, -2, -2), (0, 0, 30, 23)]


def test_filled_rectangles_are_pils(libs):
    """rect(o) against PIL.ImageDraw.rectangle(fill=...), an independent implementation with both corners inclusive: plain,
    reversed in x, in y and in both, degenerate (a point, a line), partly and wholly outside, covering the whole image; painted in
    order, so later boxes overwrite earlier ones."""
    from PIL import Image, ImageDraw
    H, W = 24, 31
    colors = [(50 + 17 * i, 254 - 13 * i, 60 + 9 * i) for i in range(len(BOXES))]
    for upto in range(1, len(BOXES) + 1):
        objs = [B.obj(*b, fill=c, flags=B.FILL) for b, c in zip(BOXES[:upto], colors)]
        objects, frames = B.tables([objs])
        got = B.render(objects, frames, H, W)[0]
        im = Image.new("RGB", (W, H))
        d = ImageDraw.Draw(im)
        for (x1, y1, x2, y2), c in zip(BOXES[:upto], colors):
            d.rectangle([min(x1, x2), min(y1, y2), max(x1, x2), max(y1, y2)], fill=c)
        # fill alone: U = 0, so out = rhe(3 T / 4) where T != 0
        T = np.asarray(im).astype(np.int64).transpose(2, 0, 1)
        assert np.array_equal(got, B.rhe_quarter(3 * T).astype(np.uint8)), upto
    X, Y = grid(H, W)
    for b in BOXES:
        im = Image.new("L", (W, H))
        ImageDraw.Draw(im).rectangle([min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])], fill=1)
        assert np.array_equal(B.rect_mask(B.obj(*b), X, Y), np.asarray(im).astype(bool)), b


def test_the_ring_is_the_three_pixel_band_without_its_outer_corners():
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0, 0],
                     [0, 1, 1, 1, 1, 1, 1, 1, 0],
                     [0, 1, 1, 1, 1, 1, 1, 1, 0],
                     [0, 1, 1, 1, 0, 1, 1, 1, 0],
                     [0, 1, 1, 1, 1, 1, 1, 1, 0],
                     [0, 1, 1, 1, 1, 1, 1, 1, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=bool)
    X, Y = grid(9, 9)
    for box in ((2, 2, 6, 6), (6, 6, 2, 2), (6, 2, 2, 6)):
        assert np.array_equal(B.ring_mask(B.obj(*box), X, Y), want), box
    # the general statement on a larger box: the band |x - edge| <= 1 around the outline, minus the four outermost corner pixels
    X, Y = grid(30, 40)
    xa, ya, xb, yb = 5, 7, 33, 21
    outer = (X >= xa - 1) & (X <= xb + 1) & (Y >= ya - 1) & (Y <= yb + 1)
    inner = (X >= xa + 2) & (X <= xb - 2) & (Y >= ya + 2) & (Y <= yb - 2)
    band = outer & ~inner
    for cx in (xa - 1, xb + 1):
        for cy in (ya - 1, yb + 1):
            band[cy, cx] = False
    assert np.array_equal(B.ring_mask(B.obj(xa, ya, xb, yb), X, Y), band)
    # through render: the outline alone comes out in line_rgb, zeros included
    objects, frames = B.tables([[B.obj(2, 2, 6, 6, line=(9, 0, 200), flags=B.OUTLINE)]])
    got = B.render(objects, frames, 9, 9)[0]
    for c, v in enumerate((9, 0, 200)):
        assert np.array_equal(got[c], want * v)


def test_the_blend_rounds_half_to_even_like_float64():
    T, U = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    want = np.rint(0.75 * T.astype(np.float64) + 0.25 * U.astype(np.float64)).astype(np.int64)
    assert np.array_equal(B.rhe_quarter(3 * T + U), want)
    assert want.max() == 255 and want.min() == 0


def test_capsules_thin_and_thick():
    X, Y = grid(9, 12)
    # a horizontal radius-1 capsule: three rows over the segment, one pixel past each end on the axis only
    m = B.capsule((3, 4), (8, 4), 4, X, Y)
    want = np.zeros((9, 12), dtype=bool)
    want[3:6, 3:9] = True
    want[4, 2] = want[4, 9] = True
    assert np.array_equal(m, want)
    # radius 1/2: the segment's own pixels; a zero-length edge is a disc
    assert np.array_equal(B.capsule((3, 4), (8, 4), 1, X, Y), (Y == 4) & (X >= 3) & (X <= 8))
    assert np.array_equal(B.capsule((5, 5), (5, 5), 4, X, Y), (np.abs(X - 5) + np.abs(Y - 5)) <= 1)
    assert np.array_equal(B.capsule((5, 5), (5, 5), 1, X, Y), (X == 5) & (Y == 5))
    # either direction covers the same pixels
    for p0, p1 in (((1, 1), (10, 7)), ((2, 8), (3, 0)), ((0, 0), (11, 8))):
        for r4 in (1, 4):
            assert np.array_equal(B.capsule(p0, p1, r4, X, Y), B.capsule(p1, p0, r4, X, Y))


# ---- the host helpers through ctypes

def test_the_class_palette(libs):
    from ctrlv_amd import _lib
    for lib in libs.values():
        rgb = (ctypes.c_uint8 * 3)()
        for i, want in enumerate(B.PALETTE):
            assert lib.ctrlv_box_class_color(i, rgb) == 0 and tuple(rgb) == want
        for bad in (-1, 11, 1 << 20):
            assert lib.ctrlv_box_class_color(bad, rgb) == -1 and "palette" in _lib.last_error(lib)
        assert lib.ctrlv_box_class_color(0, None) == -1
    assert len(B.PALETTE) == 11


def test_the_track_colour(libs):
    lib = libs[torch.bfloat16]
    rgb, again = (ctypes.c_uint8 * 3)(), (ctypes.c_uint8 * 3)()
    seen = set()
    ids = list(range(-3, 300)) + [2 ** 31, 2 ** 32 + 7, 2 ** 62, -2 ** 63]
    for seed in (0, 1, 0xDEADBEEF12345678):
        for t in ids:
            assert lib.ctrlv_box_track_color(seed, t, rgb) == 0
            assert libs[torch.float16].ctrlv_box_track_color(seed, t, again) == 0
            assert tuple(rgb) == tuple(again) == B.track_color(seed, t), (seed, t)
            assert all(50 <= v <= 254 for v in rgb)
            seen.add(tuple(rgb))
    assert len(seen) > 0.99 * 3 * len(ids)             # tracks and seeds get colours of their own
    lo = min(min(c) for c in seen)
    hi = max(max(c) for c in seen)
    assert lo == 50 and hi == 254                      # both ends of the reference's randint(50, 255) are reached
    assert lib.ctrlv_box_track_color(0, 0, None) == -1


def _project(lib, cam, loc, dims, rot_y):
    cam = np.ascontiguousarray(cam, dtype=np.float64)
    out = (ctypes.c_int16 * 16)()
    rc = lib.ctrlv_box_project_corners(cam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cam.shape[1],
                                       (ctypes.c_double * 3)(*loc), (ctypes.c_double * 3)(*dims), float(rot_y), out)
    assert rc == 0
    return np.frombuffer(out, dtype=np.int16).reshape(8, 2).copy()


def test_the_corner_projection_on_the_fixture(libs):
    cam = np.array(SCENE["cam_to_img"], dtype=np.float64)
    assert cam.shape == (3, 4)
    lib = libs[torch.bfloat16]
    for lab in SCENE["labels"]:
        for c in (cam, cam[:, :3].copy()):
            u = B.project_corners_float(c, lab["location"], lab["dimensions"], lab["rotation_y"])
            # no coordinate near an integer: a last-bit difference between two libms cannot flip a truncation
            assert float(np.abs(u - np.rint(u)).min()) > 1e-6
            want = B.project_corners(c, lab["location"], lab["dimensions"], lab["rotation_y"])
            assert np.array_equal(_project(lib, c, lab["location"], lab["dimensions"], lab["rotation_y"]), want)
            assert np.array_equal(want, np.trunc(u).astype(np.int16)) or np.abs(u).max() > B.CLAMP
    # the first object is in front of the camera and inside a KITTI-sized image: a real box, not a degenerate one
    first = B.project_corners(cam, SCENE["labels"][0]["location"], SCENE["labels"][0]["dimensions"], SCENE["labels"][0]["rotation_y"])
    assert len({tuple(p) for p in first}) == 8 and first[:, 0].min() > 0 and first[:, 0].max() < SCENE["image_size"][1]


def test_the_corner_projection_clamps_and_refuses(libs):
    from ctrlv_amd import _lib
    lib = libs[torch.bfloat16]
    cam = np.array(SCENE["cam_to_img"], dtype=np.float64)
    # a point at the camera plane: the 1e-4 divisor, far outside int16 -- clamped, not wrapped
    got = _project(lib, cam[:, :3], (3.3, 1.1, 0.00001), (0.0, 0.0, 0.0), 0.0)
    assert np.array_equal(got, B.project_corners(cam[:, :3], (3.3, 1.1, 0.00001), (0.0, 0.0, 0.0), 0.0))
    assert int(np.abs(got).max()) == B.CLAMP and int(np.abs(got).min()) == B.CLAMP
    got = _project(lib, cam, (float("nan"), 1.0, 5.0), (1.0, 1.0, 1.0), 0.3)
    assert np.array_equal(got[:, 0], np.zeros(8, dtype=np.int16))
    out = (ctypes.c_int16 * 16)()
    d3 = (ctypes.c_double * 3)(1, 1, 1)
    p = np.ascontiguousarray(cam).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for cols in (2, 5):
        assert lib.ctrlv_box_project_corners(p, cols, d3, d3, 0.0, out) == -2 and "cols" in _lib.last_error(lib)
    assert lib.ctrlv_box_project_corners(None, 4, d3, d3, 0.0, out) == -1
    assert lib.ctrlv_box_project_corners(p, 4, d3, d3, 0.0, None) == -1


# ---- refusals by name, on the host

def test_both_libraries_export_the_new_symbols_and_the_records_have_the_c_layout(libs):
    from ctrlv_amd import _lib
    from ctrlv_amd import boxes as X
    for lib in libs.values():
        assert lib.ctrlv_abi_version() == _lib.ABI_VERSION == 22
        for name in NEW:
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.BoxObject) == 64 == B.OBJECT_DTYPE.itemsize == X.OBJECT_DTYPE.itemsize
    assert ctypes.sizeof(_lib.BoxFrame) == 16 == B.FRAME_DTYPE.itemsize == X.FRAME_DTYPE.itemsize
    assert ctypes.sizeof(_lib.BoxRenderRequest) == 40
    for name in B.OBJECT_DTYPE.names:
        assert getattr(_lib.BoxObject, name).offset == B.OBJECT_DTYPE.fields[name][1] == X.OBJECT_DTYPE.fields[name][1], name
    assert _lib.BoxObject.corner.offset == 24 and _lib.BoxObject.flags.offset == 56
    for name in B.FRAME_DTYPE.names:
        assert getattr(_lib.BoxFrame, name).offset == B.FRAME_DTYPE.fields[name][1], name
    assert (_lib.BOX_FILL, _lib.BOX_OUTLINE, _lib.BOX_WIRE) == (B.FILL, B.OUTLINE, B.WIRE) == (1, 2, 4)


def test_the_render_entry_points_refuse_by_name(libs):
    from ctrlv_amd import _lib
    O, Fr, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000          # never dereferenced on the host
    for lib in libs.values():
        el = lib.ctrlv_elem_dtype()

        def render(word, code, objects=O, n_objects=3, frames=Fr, n_frames=2, Hs=37, Ws=53, out=OUT):
            rc = lib.ctrlv_render_box_frames(objects, n_objects, frames, n_frames, Hs, Ws, out, None)
            assert rc == code and word in _lib.last_error(lib), (word, rc, _lib.last_error(lib))

        render("table is null", -1, objects=None)
        render("table is null", -1, frames=None)
        render("n_objects", -1, n_objects=-1)
        render("n_frames", -2, n_frames=0)
        render("n_frames", -2, n_frames=-4)
        render("source size", -2, Hs=4097)
        render("source size", -2, Ws=4097)
        render("source size", -2, Hs=0)
        render("out_u8 is null", -1, out=None)

        def cond(word, code, objects=O, n_objects=3, frames=Fr, n_frames=2, Hs=37, Ws=53, H=16, W=24, out=OUT, dt=el, ws=WS,
                 ws_bytes=1 << 30, query=None):
            rc = lib.ctrlv_box_frames_cond(objects, n_objects, frames, n_frames, Hs, Ws, H, W, out, dt, None, ws, ws_bytes, None)
            assert rc == code and word in _lib.last_error(lib), (word, rc, _lib.last_error(lib))
            if query is not None:
                assert (lib.ctrlv_box_frames_cond_ws_bytes(n_frames, Hs, Ws, H, W) == 0) == query

        cond("table is null", -1, objects=None)
        cond("table is null", -1, frames=None)
        cond("n_objects", -1, n_objects=-2)
        cond("n_frames", -2, n_frames=0, query=True)
        cond("source size", -2, Hs=5000, query=True)
        cond("source size", -2, Ws=4097, query=True)
        cond("working size", -2, H=0, query=True)
        cond("down-scale", -2, Hs=720, Ws=1280, H=16, W=24, query=True)          # what the resize refuses, in its own words
        cond("out must be", -1, out=None)
        cond("out must be", -1, out=OUT + 4)
        cond("out_dtype", -4, dt=3 - el)                                             # the other library's element type
        cond("out_dtype", -4, dt=7)
        cond("workspace must be", -1, ws=None)
        need = lib.ctrlv_box_frames_cond_ws_bytes(2, 37, 53, 16, 24)
        assert need > 0 and need % 256 == 0
        assert need >= 2 * 3 * 37 * 53 + 2 * 3 * 16 * 24 + lib.ctrlv_resize_frames_ws_bytes(6, 37, 53, 16, 24, 2)
        cond("ws_bytes", -5, ws_bytes=need - 1, query=False)
        assert str(need) in _lib.last_error(lib)
        same = lib.ctrlv_box_frames_cond_ws_bytes(2, 37, 53, 37, 53)                # no resize: the render alone
        assert 0 < same < need and same >= 2 * 3 * 37 * 53


def test_generate_from_boxes_refuses_by_name_before_anything_else(libs):
    """The call and its workspace query alike; the valid pair reaches the next gate ("not loaded": these plans have no weights),
    which proves that every check of the request and of the tables sits in front of it."""
    from ctrlv_amd import _lib
    lib = libs[torch.bfloat16]
    unet, cn, vae, clip = _plans()
    h, h_svd = _create(lib, unet, cn, vae, clip), _create(lib, unet, None, vae, clip)
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def boxes(**over):
        b = _lib.BoxRenderRequest()
        b.objects, b.frames, b.n_objects, b.n_frames, b.src_height, b.src_width = 0x6000, 0x7000, 5, 3, 375, 1242
        for k, v in over.items():
            setattr(b, k, v)
        return b

    def refused(r, b, word, pipe=h, code=None):
        assert lib.ctrlv_pipeline_from_boxes_workspace_bytes(pipe, ctypes.byref(r), ctypes.byref(b) if b else None) == 0
        m1 = _lib.last_error(lib)
        rc = lib.ctrlv_pipeline_generate_from_boxes(pipe, ctypes.byref(r), ctypes.byref(b) if b else None, ws, 1 << 40, None)
        m2 = _lib.last_error(lib)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        assert code is None or rc == code, (word, rc)

    ok = lambda **kw: _request(_lib, keep, cond=None, **kw)        # noqa: E731
    refused(ok(), boxes(), "not loaded")
    refused(ok(), boxes(src_height=128, src_width=192), "not loaded")                      # the same size: no resize
    refused(_request(_lib, keep), boxes(), "cond is set together with boxes", code=-1)
    refused(ok(), None, "null box render request", code=-1)
    refused(ok(), boxes(), "no ControlNet", pipe=h_svd, code=-1)
    res = boxes()
    res.reserved[1] = 1
    refused(ok(), res, "reserved", code=-1)
    refused(ok(), boxes(n_frames=4), "n_frames", code=-2)
    refused(ok(n_clips=2), boxes(), "n_frames", code=-2)
    refused(ok(num_frames=33), boxes(), "num_frames")                                       # the request, as generate validates it
    refused(ok(), boxes(objects=None), "table is null", code=-1)
    refused(ok(), boxes(frames=None), "table is null", code=-1)
    refused(ok(), boxes(n_objects=-1), "n_objects", code=-1)
    refused(ok(), boxes(src_height=4097), "source size", code=-2)
    refused(ok(), boxes(src_height=128 * 17), "down-scale", code=-2)
    assert lib.ctrlv_pipeline_destroy(h) == 0 and lib.ctrlv_pipeline_destroy(h_svd) == 0


def test_the_python_layer_keeps_boxes_and_cond_apart():
    from ctrlv_amd.plan import PipelinePlan
    plan = PipelinePlan.__new__(PipelinePlan)          # no handle: the check under test comes before anything is touched
    img = torch.zeros(1, 128, 192, 3, dtype=torch.uint8)
    lat = torch.zeros(1, 3, 4, 16, 24)
    with pytest.raises(ValueError, match="mutually exclusive"):
        PipelinePlan.generate(plan, img, lat, [1.0, 0.0], [0.5], cond=torch.zeros(1, 3, 3, 128, 192), boxes=object(),
                              source_size=(375, 1242))
    with pytest.raises(ValueError, match="mutually exclusive"):
        PipelinePlan.predict_boxes(plan, img, lat, [1.0, 0.0], [0.5], torch.zeros(1, 3, 3, 128, 192), boxes=object(),
                                   source_size=(375, 1242))


# ---- BoxTable.from_labels against hand-built records

def _records(table):
    objects = table.objects.numpy().view(B.OBJECT_DTYPE).reshape(-1)
    frames = table.frames.numpy().view(B.FRAME_DTYPE).reshape(-1)
    return objects, frames


def test_from_labels_builds_the_documented_records(libs):
    from ctrlv_amd.boxes import BoxTable
    labs = SCENE["labels"]
    cam = np.array(SCENE["cam_to_img"])
    neg = dict(labs[1], bbox=[-3.7, -0.4, 10.9, 7.5])                 # int() truncates toward zero: -3, 0, 10, 7
    clips = [[[labs[0], labs[1]], [], [neg]], [[labs[2]], [labs[3], labs[0], labs[1]], [labs[2]]]]
    # without a camera: FILL | OUTLINE, no corners
    t = BoxTable.from_labels(clips, seed=9)
    objects, frames = _records(t)
    assert (t.n_clips, t.num_frames, t.n_frames, t.n_objects) == (2, 3, 6, 8)
    assert [tuple(f) for f in frames] == [(0, 2, 0, 0), (2, 0, 0, 0), (2, 1, 0, 0), (3, 1, 0, 0), (4, 3, 0, 0), (7, 1, 0, 0)]
    flat = [labs[0], labs[1], neg, labs[2], labs[3], labs[0], labs[1], labs[2]]
    for o, lab in zip(objects, flat):
        assert (o["x1"], o["y1"], o["x2"], o["y2"]) == tuple(int(v) for v in lab["bbox"])
        assert tuple(o["fill_rgb"]) == B.track_color(9, lab["trackID"]) + (0,)
        assert tuple(o["line_rgb"]) == B.PALETTE[lab["id_type"]] + (0,)
        assert o["flags"] == B.FILL | B.OUTLINE and o["reserved"] == 0 and not o["corner"].any()
    assert (objects[2]["x1"], objects[2]["y1"], objects[2]["x2"], objects[2]["y2"]) == (-3, 0, 10, 7)
    # another seed: other track colours, the same class colours
    o2, _ = _records(BoxTable.from_labels(clips, seed=10))
    assert not np.array_equal(o2["fill_rgb"], objects["fill_rgb"]) and np.array_equal(o2["line_rgb"], objects["line_rgb"])
    # with a camera: FILL | WIRE and the projected corners; is_gt picks rotation_y, else alpha and the viewing angle
    for is_gt in (True, False):
        oc, fc = _records(BoxTable.from_labels(clips, cam_to_img=cam, seed=9, is_gt=is_gt))
        assert np.array_equal(fc, frames)
        for o, lab in zip(oc, flat):
            loc = lab["location"]
            rot = lab["rotation_y"] if is_gt else lab["alpha"] / 180 * np.pi + np.arctan(loc[0] / loc[2])
            assert o["flags"] == B.FILL | B.WIRE
            assert np.array_equal(o["corner"], B.project_corners(cam, loc, lab["dimensions"], rot))
    # trajectory_last: frame F - 1 of every clip has kind 1 and the disc centre int((x1 + x2) / 2), int((y1 + y2) / 2) on the floats
    ot, ft = _records(BoxTable.from_labels(clips, cam_to_img=cam, seed=9, trajectory_last=True))
    assert [int(f["kind"]) for f in ft] == [0, 0, 1, 0, 0, 1]
    for i in (2, 7):
        x1, y1, x2, y2 = flat[i]["bbox"]
        assert tuple(ot[i]["corner"][0]) == (int((x1 + x2) / 2), int((y1 + y2) / 2)) and not ot[i]["corner"][1:].any()
    assert tuple(ot[2]["corner"][0]) == (3, 3)                        # (-3.7 + 10.9) / 2 = 3.6, (-0.4 + 7.5) / 2 = 3.55
    oc, _ = _records(BoxTable.from_labels(clips, cam_to_img=cam, seed=9))
    assert np.array_equal(ot[0]["corner"], oc[0]["corner"])           # the other frames are box frames as before
    # a table without any object still has a record to point at, and draws nothing
    empty = BoxTable.from_labels([[[], []]])
    oe, fe = _records(empty)
    assert empty.n_objects == 1 and oe[0]["flags"] == 0 and [tuple(f) for f in fe] == [(0, 0, 0, 0), (0, 0, 0, 0)]
    assert BoxTable.from_labels(clips).clip(1).frames.tolist() == t.frames[3:].tolist()
