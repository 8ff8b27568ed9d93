"""The box predictor, the kernels between the stages and the boxes-to-video chain (include/ctrlv_hip.h:
ctrlv_pipeline_predict_boxes, ctrlv_box_frames_post, ctrlv_mask_counts, ctrlv_pipeline_boxes_to_video) where no GPU is needed:
the symbols, the struct mirrors, the host-side validation -- every refusal names what it refuses and comes before anything would
be launched --, the metric from recorded counts against the reference's own triples, and the route predicate."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import box_chain_utils as B
from tests.test_pipeline_plan_cpu import CLIP_CFG, VAE_CFG, _request

NEW = ("ctrlv_pipeline_boxes_workspace_bytes", "ctrlv_pipeline_predict_boxes", "ctrlv_box_frames_post_ws_bytes",
       "ctrlv_box_frames_post", "ctrlv_mask_counts", "ctrlv_pipeline_chain_workspace_bytes", "ctrlv_pipeline_boxes_to_video")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


def _plans(device="cpu", dtype=torch.bfloat16):
    """Unloaded plans of the tiny models: create needs no GPU."""
    import ctrlv_ref as R
    from ctrlv_amd.plan import ClipPlan, Plan, VaePlan
    cfg = dict(R.TINY_CONFIG)
    ccfg = {k: v for k, v in cfg.items() if k not in ("out_channels", "up_block_types")}
    return (Plan("unet", cfg, device, dtype=dtype), Plan("controlnet", ccfg, device, dtype=dtype),
            VaePlan(VAE_CFG, device, dtype=dtype), ClipPlan(CLIP_CFG, device, dtype=dtype))


@pytest.fixture(scope="module")
def plans(libs):
    return _plans()


def _create(lib, unet, cn, vae, clip, device=0):
    h = ctypes.c_void_p()
    rc = lib.ctrlv_pipeline_create(unet._h, cn._h if cn else None, vae._h, clip._h, device, ctypes.byref(h))
    assert rc == 0 and h.value
    return h


def test_both_libraries_export_the_new_symbols_at_abi_22(libs):
    from ctrlv_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read(), flags=re.S)
    for dt, lib in libs.items():
        assert lib.ctrlv_abi_version() == 22 == _lib.ABI_VERSION
        for name in NEW:
            assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", header), name
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (dt, name)


def _c_fields(struct):
    src = open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read()
    body = src[src.index("typedef struct %s {" % struct):src.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head = decl.split(",")[0].strip()
        ctype = " ".join(head.split()[:-1]) + ("*" if head.split()[-1].startswith("*") else "")
        for part in decl.split(","):
            out.append((part.strip().split()[-1].lstrip("*"), ctype))
    return out


def test_the_struct_mirrors_have_the_c_layout():
    """Names in header order, and the offsets of the C struct's natural layout (each field aligned to its size, a nested struct
    to its widest member, the size rounded up to the alignment)."""
    from ctrlv_amd import _lib
    sizes = {"int32_t": 4, "float": 4, "const void*": 8, "void*": 8, "ctrlv_clip_request": ctypes.sizeof(_lib.ClipRequest),
             "ctrlv_box_condition": 24}
    for struct, mirror in (("ctrlv_box_condition", _lib.BoxCondition), ("ctrlv_two_stage_request", _lib.TwoStageRequest)):
        fields = _c_fields(struct)
        assert [n for n, _ in fields] == [f[0] for f in mirror._fields_], struct
        off = 0
        for name, ctype in fields:
            size = sizes[ctype]
            align = min(size, 8)
            off = (off + align - 1) // align * align
            assert getattr(mirror, name).offset == off, (struct, name, off)
            off += size
        assert ctypes.sizeof(mirror) == (off + 7) // 8 * 8, struct
    assert ctypes.sizeof(_lib.BoxCondition) == 24


def _box(_lib, **over):
    bc = _lib.BoxCondition()
    bc.frames, bc.channels, bc.dtype, bc.num_cond_frames = 0x6000, 3, 0, 1
    for k, v in over.items():
        setattr(bc, k, v)
    return bc


def test_predict_boxes_refuses_by_name_before_anything_else(libs, plans):
    """predict_boxes and its workspace query alike; the valid request reaches the next gate ("not loaded": these plans have no
    weights), which proves that every field check sits in front of it."""
    from ctrlv_amd import _lib
    lib = libs[torch.bfloat16]
    unet, cn, vae, clip = plans
    h_cn, h = _create(lib, unet, cn, vae, clip), _create(lib, unet, None, vae, clip)
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def refused(r, bc, word, pipe=h, code=None):
        assert lib.ctrlv_pipeline_boxes_workspace_bytes(pipe, ctypes.byref(r), ctypes.byref(bc) if bc else None) == 0
        m1 = _lib.last_error(lib)
        rc = lib.ctrlv_pipeline_predict_boxes(pipe, ctypes.byref(r), ctypes.byref(bc) if bc else None, ws, 1 << 40, None)
        m2 = _lib.last_error(lib)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        assert code is None or rc == code, (word, rc)

    ok = lambda **kw: _request(_lib, keep, cond=None, **kw)        # noqa: E731
    refused(ok(), _box(_lib), "not loaded")
    refused(ok(), _box(_lib, channels=4, dtype=2, num_cond_frames=0), "not loaded")
    refused(ok(), _box(_lib, num_cond_frames=3), "not loaded")                            # K = F
    refused(_request(_lib, keep), _box(_lib), "has a ControlNet", pipe=h_cn, code=-1)
    refused(ok(), _box(_lib), "has a ControlNet", pipe=h_cn, code=-1)
    refused(_request(_lib, keep), _box(_lib), "cond is set", code=-1)
    refused(ok(), None, "null box condition", code=-1)
    refused(ok(num_frames=33), _box(_lib), "num_frames")                                  # the request, as generate validates it
    refused(ok(decode_chunk=0), _box(_lib), "decode_chunk")
    for K in (-1, 4):
        refused(ok(), _box(_lib, num_cond_frames=K), "num_cond_frames", code=-2)
    for ch in (0, 1, 5, 8):
        refused(ok(), _box(_lib, channels=ch), "channels", code=-2)
    for dt in (-1, 3):
        refused(ok(), _box(_lib, dtype=dt), "dtype", code=-4)
    refused(ok(), _box(_lib, frames=None), "frames is null", code=-1)
    refused(ok(), _box(_lib, reserved=1), "reserved", code=-1)
    assert lib.ctrlv_pipeline_destroy(h) == 0 and lib.ctrlv_pipeline_destroy(h_cn) == 0


def test_the_chain_refuses_by_name_before_anything_else(libs, plans):
    from ctrlv_amd import _lib
    lib, lib16 = libs[torch.bfloat16], libs[torch.float16]
    unet, cn, vae, clip = plans
    hb, hv = _create(lib, unet, None, vae, clip), _create(lib, unet, cn, vae, clip)
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def chain(boxes=None, video=None, **over):
        q = _lib.TwoStageRequest()
        q.boxes = _request(_lib, keep, **dict(dict(cond=None), **(boxes or {})))
        q.video = _request(_lib, keep, **dict(dict(cond=None), **(video or {})))
        q.box_cond = _box(_lib)
        q.clean_threshold = 50.0
        for k, v in over.items():
            setattr(q, k, v)
        return q

    def refused(q, word, pb=hb, pv=hv, code=None, use=lib):
        assert use.ctrlv_pipeline_chain_workspace_bytes(pb, pv, ctypes.byref(q)) == 0
        m1 = _lib.last_error(use)
        rc = use.ctrlv_pipeline_boxes_to_video(pb, pv, ctypes.byref(q), ws, 1 << 40, None)
        m2 = _lib.last_error(use)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        assert code is None or rc == code, (word, rc)

    refused(chain(), "not loaded")
    refused(chain(boxes=dict(out_frames=0x7000)), "not loaded")
    for field, value in (("n_clips", 2), ("num_frames", 2), ("height", 256), ("width", 128)):
        refused(chain(video={field: value}), "differ in geometry", code=-2)
    refused(chain(video=dict(cond=0x2000)), "video.cond", code=-1)
    refused(chain(boxes=dict(cond=0x2000)), "cond is set", code=-1)
    refused(chain(reserved=3), "reserved", code=-1)
    refused(chain(box_cond=_box(_lib, num_cond_frames=9)), "num_cond_frames", code=-2)
    refused(chain(video=dict(decode_chunk=0)), "decode_chunk")
    refused(chain(), "has a ControlNet", pb=hv, code=-1)                    # stage 1 on a ControlNet pipeline
    refused(chain(), "no ControlNet", pv=hb, code=-1)                       # stage 2 without one
    refused(chain(), "null pipeline", pb=None, code=-1)
    # the other device: plans and pipelines of device 1 are host objects like the others
    others = _plans("cuda:1")
    hb1 = _create(lib, others[0], None, others[2], others[3], device=1)
    refused(chain(), "different devices", pb=hb1, code=-1)
    # the other library: its handles are refused by both
    others16 = _plans(dtype=torch.float16)
    hb16 = _create(lib16, others16[0], None, others16[2], others16[3])
    refused(chain(), "this library", pb=hb16, code=-1)
    refused(chain(), "this library", pb=hb, pv=hv, code=-1, use=lib16)
    assert lib16.ctrlv_pipeline_destroy(hb16) == 0
    for h in (hb, hv, hb1):
        assert lib.ctrlv_pipeline_destroy(h) == 0


def test_the_kernels_between_the_stages_validate_on_the_host(libs):
    from ctrlv_amd import _lib
    for lib in libs.values():
        p = ctypes.c_void_p(0x1000)
        assert lib.ctrlv_box_frames_post_ws_bytes(2, 5) == 40
        assert lib.ctrlv_box_frames_post_ws_bytes(0, 5) == 0 and "positive" in _lib.last_error(lib)
        post = lambda *a: lib.ctrlv_box_frames_post(*a, None)        # noqa: E731
        assert post(None, 1, 3, 8, 8, 50.0, p, p, p, p, 12) == -1 and "frames is null" in _lib.last_error(lib)
        assert post(p, 1, 3, 8, 8, 50.0, None, None, None, p, 12) == -1 and "outputs are null" in _lib.last_error(lib)
        assert post(p, 1, 0, 8, 8, 50.0, p, None, None, None, 0) == -2 and "positive" in _lib.last_error(lib)
        assert post(p, 2, 3, 8, 8, 50.0, None, None, p, p, 23) == -5 and "ws_bytes" in _lib.last_error(lib)
        assert post(p, 2, 3, 8, 8, 50.0, None, None, p, None, 24) == -1 and "ws" in _lib.last_error(lib)
        assert lib.ctrlv_mask_counts(p, None, 1, 3, 8, 8, p, None) == -1 and "null" in _lib.last_error(lib)
        assert lib.ctrlv_mask_counts(p, p, 1, 3, 0, 8, p, None) == -2 and "positive" in _lib.last_error(lib)


def test_the_restated_cleanup_is_the_references(libs):
    """tests/box_chain_utils.cleanup_numpy, which the GPU test of ctrlv_box_frames_post applies where a golden input is not
    exact in the element type, gives the reference's recorded bytes on every golden input (the pixel at exactly the threshold
    included)."""
    for lib in libs.values():
        assert lib.ctrlv_box_frames_post is not None           # (the kernel the restatement stands beside)
    for name in B.CLEAN_CASES:
        assert np.array_equal(B.cleanup_numpy(B.G[name + "_y"]), B.G[name + "_u8"]), name


def test_binary_mask_iou_from_recorded_counts_is_the_references():
    from ctrlv_amd import metrics
    for name in B.IOU_CASES:
        counts = B.G[f"iou_{name}_counts"]
        for row, key in ((0, "all"), (1, "first_last")):
            got, want = metrics.iou_from_counts(*counts[row]), tuple(B.G[f"iou_{name}_{key}"])
            assert got == want, (name, key, got, want)
    assert metrics.iou_from_counts(0, 0, 0) == (1, 1, 1)
    assert metrics.iou_from_counts(0, 5, 0) == (0.0, 0.0, 1) and metrics.iou_from_counts(5, 0, 0) == (0.0, 1, 0.0)


def test_the_route_predicate_takes_box_frames_only_on_the_plan_route():
    from PIL import Image
    from ctrlv_amd.pipelines.pipeline_utils import pipeline_route
    im = Image.new("RGB", (16, 8))
    boxes = torch.zeros(1, 3, 3, 8, 16)
    on = {"CTRLV_PIPELINE": "plan"}
    assert pipeline_route(im, None, "pt", True, env=on, bbox_images=boxes) == "plan"
    assert pipeline_route(im, None, "pt", True, env=on) == "plan"
    asked = []
    serve = lambda: (asked.append(1), True)[1]        # noqa: E731
    assert pipeline_route(im, None, "pt", serve, env={}, bbox_images=boxes) == "python"            # unset: as before
    assert pipeline_route(im, None, "pt", serve, env={"CTRLV_PIPELINE": "1"}, bbox_images=boxes) == "python"
    assert pipeline_route(im, None, "pt", serve, env=on, bbox_images=boxes.numpy()) == "python"    # not a tensor
    assert pipeline_route(im, None, "pt", serve, env=on, bbox_images=[boxes]) == "python"
    assert pipeline_route(im, lambda *a: {}, "pt", serve, env=on, bbox_images=boxes) == "python"   # a per-step callback
    assert pipeline_route(torch.zeros(1, 3, 8, 16), None, "pt", serve, env=on, bbox_images=boxes) == "python"
    assert not asked
    assert pipeline_route(im, None, "pt", False, env=on, bbox_images=boxes) == "python"
