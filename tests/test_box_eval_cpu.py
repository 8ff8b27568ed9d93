"""Best-of-N box candidates and the boundary F-measure (include/ctrlv_hip.h: ctrlv_best_candidate, ctrlv_gather_clips,
ctrlv_pipeline_best_boxes, ctrlv_pipeline_best_boxes_to_video, ctrlv_boundary_radius, ctrlv_boundary_counts) where no GPU is needed:
the symbols, the struct mirrors, every host-side refusal by name, the radius, the numpy restatement of the boundary counts
(tests/box_eval_ref.py) against known answers, the luma mask rule against PIL, and the host restatement of the best-of-N rule."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from tests import box_eval_ref as E
from tests.test_box_chain_cpu import _box, _c_fields, _create, _plans
from tests.test_pipeline_plan_cpu import _request

NEW = ("ctrlv_best_candidate", "ctrlv_gather_clips", "ctrlv_pipeline_best_boxes_workspace_bytes", "ctrlv_pipeline_best_boxes",
       "ctrlv_pipeline_best_chain_workspace_bytes", "ctrlv_pipeline_best_boxes_to_video", "ctrlv_boundary_radius",
       "ctrlv_boundary_counts")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    g.build()
    from ctrlv_amd import _lib
    return {torch.bfloat16: _lib.load(torch.bfloat16), torch.float16: _lib.load(torch.float16)}


@pytest.fixture(scope="module")
def plans(libs):
    return _plans()


def test_both_libraries_export_the_new_symbols_at_abi_22(libs):
    from ctrlv_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctrlv_hip.h")).read(), flags=re.S)
    for dt, lib in libs.items():
        assert lib.ctrlv_abi_version() == 22 == _lib.ABI_VERSION
        for name in NEW:
            assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", header), name
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (dt, name)
    assert "box_eval.hip" in g.HIP_SOURCES


def test_the_struct_mirrors_have_the_c_layout():
    """Names in header order and the offsets of the C struct's natural layout, by the method of tests/test_box_chain_cpu.py; the
    existing request structs keep their sizes."""
    from ctrlv_amd import _lib
    sizes = {"int32_t": 4, "float": 4, "ctrlv_clip_request": ctypes.sizeof(_lib.ClipRequest), "ctrlv_box_condition": 24,
             "ctrlv_best_boxes_request": ctypes.sizeof(_lib.BestBoxesRequest)}
    for struct, mirror in (("ctrlv_best_boxes_request", _lib.BestBoxesRequest), ("ctrlv_best_chain_request", _lib.BestChainRequest)):
        fields = _c_fields(struct)
        assert [n for n, _ in fields] == [f[0] for f in mirror._fields_], struct
        off = 0
        for name, ctype in fields:
            size = 8 if ctype.endswith("*") else sizes[ctype]
            align = min(size, 8)
            off = (off + align - 1) // align * align
            assert getattr(mirror, name).offset == off, (struct, name, off)
            off += size
        assert ctypes.sizeof(mirror) == (off + 7) // 8 * 8, struct
    assert ctypes.sizeof(_lib.BestBoxesRequest) == 96
    assert ctypes.sizeof(_lib.BoxCondition) == 24 and ctypes.sizeof(_lib.SeedRequest) == 64
    assert ctypes.sizeof(_lib.TwoStageRequest) == 2 * ctypes.sizeof(_lib.ClipRequest) + 24 + 16


def _best(_lib, keep, C=3, cands=None, **over):
    rs = [_request(_lib, keep, **dict(dict(cond=None, out_frames_u8=None), **((cands or {}).get(c, {})))) for c in range(C)]
    arr = (_lib.ClipRequest * max(C, 1))(*rs) if C > 0 else (_lib.ClipRequest * 1)()
    keep += [arr, rs]
    q = _lib.BestBoxesRequest()
    q.n_candidates, q.candidates, q.box_cond = C, arr, _box(_lib)
    q.gt_u8, q.clean_threshold = 0x8000, 50.0
    for k, v in over.items():
        setattr(q, k, v)
    return q


def test_best_boxes_refuses_by_name_before_anything_else(libs, plans):
    """The call and its size query alike, with unloaded plans and fake pointers; a valid request reaches the next gate ("not
    loaded"), which proves that every field check sits in front of it."""
    from ctrlv_amd import _lib
    lib, lib16 = libs[torch.bfloat16], libs[torch.float16]
    unet, cn, vae, clip = plans
    h, h_cn = _create(lib, unet, None, vae, clip), _create(lib, unet, cn, vae, clip)
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def refused(q, word, pipe=h, code=None, use=lib):
        assert use.ctrlv_pipeline_best_boxes_workspace_bytes(pipe, ctypes.byref(q) if q is not None else None) == 0
        m1 = _lib.last_error(use)
        rc = use.ctrlv_pipeline_best_boxes(pipe, ctypes.byref(q) if q is not None else None, ws, 1 << 40, None)
        m2 = _lib.last_error(use)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        assert code is None or rc == code, (word, rc)

    refused(_best(_lib, keep), "not loaded")
    refused(_best(_lib, keep, C=1), "not loaded")
    refused(_best(_lib, keep, C=8, out_pt=0x9000, out_counts=0xA000, out_winner=0xB004), "not loaded")
    # the candidates may differ in guidance, steps and latents
    refused(_best(_lib, keep, cands={1: dict(max_guidance=5.0, latents=0x3100), 2: dict(max_guidance=1.0)}), "not loaded")
    for C in (0, 9, -1):
        refused(_best(_lib, keep, C=C), "n_candidates", code=-2)
    refused(_best(_lib, keep, candidates=None), "candidates array is null", code=-1)
    refused(_best(_lib, keep, gt_u8=None), "gt_u8 is null", code=-1)
    refused(_best(_lib, keep, reserved=1), "reserved", code=-1)
    refused(_best(_lib, keep, reserved2=1), "reserved", code=-1)
    for bad in (float("nan"), float("inf")):
        refused(_best(_lib, keep, clean_threshold=bad), "clean_threshold", code=-1)
    for field, value in (("n_clips", 2), ("num_frames", 2), ("height", 256), ("width", 128)):
        refused(_best(_lib, keep, cands={2: {field: value}}), "differ in geometry", code=-2)
    refused(_best(_lib, keep, cands={1: dict(out_frames=0x7000)}), "candidate 1 has out_frames", code=-1)
    refused(_best(_lib, keep, cands={2: dict(out_frames_u8=0x7000)}), "candidate 2 has out_frames", code=-1)
    refused(_best(_lib, keep, out_counts=0xA004), "out_counts", code=-1)
    refused(_best(_lib, keep, out_winner=0xB002), "out_winner", code=-1)
    # what predict_boxes refuses
    refused(_best(_lib, keep), "has a ControlNet", pipe=h_cn, code=-1)
    refused(_best(_lib, keep, cands={1: dict(cond=0x2000)}), "cond is set", code=-1)
    refused(_best(_lib, keep, box_cond=_box(_lib, num_cond_frames=9)), "num_cond_frames", code=-2)
    refused(_best(_lib, keep, box_cond=_box(_lib, reserved=1)), "reserved", code=-1)
    refused(_best(_lib, keep, cands={2: dict(decode_chunk=0)}), "decode_chunk")
    refused(_best(_lib, keep, cands={0: dict(num_steps=0)}), "num_steps")
    refused(_best(_lib, keep), "null pipeline", pipe=None, code=-1)
    refused(None, "null request", code=-1)
    refused(_best(_lib, keep), "this library", code=-1, use=lib16)
    assert lib.ctrlv_pipeline_destroy(h) == 0 and lib.ctrlv_pipeline_destroy(h_cn) == 0


def test_the_best_chain_refuses_by_name_before_anything_else(libs, plans):
    from ctrlv_amd import _lib
    lib, lib16 = libs[torch.bfloat16], libs[torch.float16]
    unet, cn, vae, clip = plans
    hb, hv = _create(lib, unet, None, vae, clip), _create(lib, unet, cn, vae, clip)
    keep = []
    ws = ctypes.c_void_p(0x100000)

    def chain(video=None, reserved=0, **best):
        q = _lib.BestChainRequest()
        q.boxes = _best(_lib, keep, **best)
        q.video = _request(_lib, keep, **dict(dict(cond=None), **(video or {})))
        q.reserved = reserved
        return q

    def refused(q, word, pb=hb, pv=hv, code=None, use=lib):
        assert use.ctrlv_pipeline_best_chain_workspace_bytes(pb, pv, ctypes.byref(q)) == 0
        m1 = _lib.last_error(use)
        rc = use.ctrlv_pipeline_best_boxes_to_video(pb, pv, ctypes.byref(q), ws, 1 << 40, None)
        m2 = _lib.last_error(use)
        assert rc < 0 and word in m1 and word in m2, (word, rc, m1, m2)
        assert code is None or rc == code, (word, rc)

    refused(chain(), "not loaded")
    refused(chain(C=1), "not loaded")
    refused(chain(out_cond=0x9000), "not loaded")
    for field, value in (("n_clips", 2), ("num_frames", 2), ("height", 256), ("width", 128)):
        refused(chain(video={field: value}), "differ in geometry", code=-2)
        refused(chain(cands={1: {field: value}}), "differ in geometry", code=-2)
    refused(chain(video=dict(cond=0x2000)), "video.cond", code=-1)
    refused(chain(reserved=3), "reserved", code=-1)
    refused(chain(C=9), "n_candidates", code=-2)
    refused(chain(gt_u8=None), "gt_u8 is null", code=-1)
    refused(chain(cands={0: dict(out_frames=0x7000)}), "candidate 0 has out_frames", code=-1)
    refused(chain(clean_threshold=float("nan")), "clean_threshold", code=-1)
    refused(chain(video=dict(decode_chunk=0)), "decode_chunk")
    refused(chain(), "has a ControlNet", pb=hv, code=-1)                    # stage 1 on a ControlNet pipeline
    refused(chain(), "no ControlNet", pv=hb, code=-1)                       # stage 2 without one
    refused(chain(), "null pipeline", pb=None, code=-1)
    others = _plans("cuda:1")
    hb1 = _create(lib, others[0], None, others[2], others[3], device=1)
    refused(chain(), "different devices", pb=hb1, code=-1)
    others16 = _plans(dtype=torch.float16)
    hb16 = _create(lib16, others16[0], None, others16[2], others16[3])
    refused(chain(), "this library", pb=hb16, code=-1)
    refused(chain(), "this library", code=-1, use=lib16)
    assert lib16.ctrlv_pipeline_destroy(hb16) == 0
    for h in (hb, hv, hb1):
        assert lib.ctrlv_pipeline_destroy(h) == 0


def test_the_kernels_validate_on_the_host(libs):
    from ctrlv_amd import _lib
    for lib in libs.values():
        p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
        err = lambda: _lib.last_error(lib)        # noqa: E731
        best = lambda *a: lib.ctrlv_best_candidate(*a, None)        # noqa: E731
        assert best(None, 1, 3, p) == -1 and "null" in err()
        assert best(p, 1, 3, None) == -1 and "null" in err()
        assert best(odd, 1, 3, p) == -1 and "8-byte" in err()
        assert best(p, 1, 3, ctypes.c_void_p(0x1002)) == -1 and "4-byte" in err()
        for C in (0, 9):
            assert best(p, 1, C, p) == -2 and "C=" in err()
        assert best(p, 0, 3, p) == -2 and "positive" in err()
        gather = lambda *a: lib.ctrlv_gather_clips(*a, None)        # noqa: E731
        assert gather(None, p, 1, 3, 16, p) == -1 and "null" in err()
        assert gather(p, None, 1, 3, 16, p) == -1 and "null" in err()
        assert gather(p, p, 1, 3, 16, None) == -1 and "null" in err()
        assert gather(p, ctypes.c_void_p(0x1002), 1, 3, 16, p) == -1 and "4-byte" in err()
        for C in (0, 9):
            assert gather(p, p, 1, C, 16, p) == -2 and "C=" in err()
        assert gather(p, p, 0, 3, 16, p) == -2 and "positive" in err()
        assert gather(p, p, 1, 3, 0, p) == -2 and "bytes_per_clip" in err()
        bc = lambda *a: lib.ctrlv_boundary_counts(*a, None)        # noqa: E731
        assert bc(None, p, 1, 1, 8, 8, 0, 1, p) == -1 and "null" in err()
        assert bc(p, p, 1, 1, 8, 8, 0, 1, None) == -1 and "null" in err()
        assert bc(p, p, 1, 1, 8, 8, 0, 1, odd) == -1 and "8-byte" in err()
        for r in (0, 33, -1):
            assert bc(p, p, 1, 1, 8, 8, 0, r, p) == -2 and "radius" in err()
        for mode in (-1, 2):
            assert bc(p, p, 1, 1, 8, 8, mode, 1, p) == -2 and "mask_mode" in err()
        for shape in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -3)):
            assert bc(p, p, *shape, 0, 1, p) == -2 and "positive" in err()
        assert bc(p, p, 1, 1, 8, 1920, 0, 32, p) == -2 and "LDS" in err()            # 30 words a row at radius 32
        assert bc(p, p, 1, 1, 8, 1 << 20, 0, 1, p) == -2 and "LDS" in err()
        assert bc(p, p, 65536, 32768, 1, 1, 0, 1, p) == -2 and "workgroups" in err()


def test_boundary_radius(libs):
    from ctrlv_amd import _lib, metrics
    want = {(576, 1024): 10, (320, 512): 5, (128, 192): 2, (37, 70): 1, (75, 100): 1, (150, 200): 2, (300, 400): 4}
    for lib in libs.values():
        for (H, W), r in want.items():
            assert lib.ctrlv_boundary_radius(H, W, 0.008) == r == E.radius(H, W), (H, W)
        assert lib.ctrlv_boundary_radius(37, 70, 3.0) == 3 and lib.ctrlv_boundary_radius(576, 1024, 1.0) == 1
        assert lib.ctrlv_boundary_radius(100, 100, 0.02) == 3                                 # ceil(2.83)
        assert lib.ctrlv_boundary_radius(37, 70, 2.5) < 0 and "integer" in _lib.last_error(lib)
        assert lib.ctrlv_boundary_radius(0, 70, 0.008) < 0 and "positive" in _lib.last_error(lib)
        for bad in (float("nan"), float("inf"), -0.5):
            assert lib.ctrlv_boundary_radius(37, 70, bad) < 0 and "bound_th" in _lib.last_error(lib)
    assert metrics.boundary_radius(320, 512) == 5 and metrics.boundary_radius(320, 512, 7) == 7
    with pytest.raises(ValueError, match="integer"):
        metrics.boundary_radius(37, 70, 2.5)


def test_the_restatement_gives_the_known_answers():
    """Counts computed once from an independent numpy restatement with scipy's binary_dilation (rectangles on 37 x 70; case B
    touches the last row and column), and the F-measure formed from them."""
    from ctrlv_amd import metrics
    for (case, r), want in E.KNOWN.items():
        G, P = (E.rect(*q) for q in E.RECTS[case])
        got = E.frame_counts(G, P, r)
        assert got == want, (case, r, got)
        u8 = E.boundary_counts(E.as_u8(G)[None, None], E.as_u8(P)[None, None], 1, r)
        assert tuple(u8[0, 0]) == want
        if (case, r) in E.KNOWN_F:
            assert metrics.f_from_counts(*got)[0] == pytest.approx(E.KNOWN_F[(case, r)], rel=0, abs=1e-15), (case, r)
    full = E.frame_counts(np.ones((E.H0, E.W0), bool), E.rect(*E.RECTS["A"][1]), 2)
    assert full == (102, 0, 0, 0)                              # a ground truth without a boundary
    # precision 0, recall 1.  The feature request's table gives F = 1 for this row; its own arithmetic -- and the reference's
    # f_measure, FandJ.py:140-154 -- give 2 p r / (p + r) = 0 for p = 0.  The arithmetic is what is implemented and asserted.
    assert metrics.f_from_counts(*full) == (0.0, 0.0, 1.0)
    for H, W in ((1, 1), (1, 9), (9, 1)):                      # degenerate shapes: the corner alone has no boundary
        assert E.frame_counts(np.ones((H, W), bool), np.zeros((H, W), bool), 1) == (0, 0, 0, 0)
    one = np.zeros((1, 9), bool)
    one[0, 3:5] = True
    assert E.boundary_map(one).tolist() == [[False, False, True, False, True, False, False, False, False]]


def test_f_from_counts_special_cases():
    from ctrlv_amd import metrics
    assert metrics.f_from_counts(0, 7, 0, 0) == (0.0, 1.0, 0.0)          # no predicted boundary: precision 1, recall 0
    assert metrics.f_from_counts(7, 0, 0, 0) == (0.0, 0.0, 1.0)          # no true boundary: precision 0, recall 1
    assert metrics.f_from_counts(0, 0, 0, 0) == (1.0, 1.0, 1.0)
    assert metrics.f_from_counts(5, 8, 0, 0) == (0.0, 0.0, 0.0)          # precision + recall = 0
    f, p, r = metrics.f_from_counts(102, 94, 48, 53)
    assert (p, r) == (48 / 102, 53 / 94) and f == 2 * p * r / (p + r)


def test_the_luma_mask_rule_is_pils():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    px = np.concatenate([rng.integers(0, 256, (4000, 3)), rng.integers(0, 6, (4000, 3)),
                         [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 0, 4), (0, 0, 5), (3, 0, 0), (1, 0, 3), (0, 0, 0)]]).astype(np.uint8)
    img = px.reshape(1, -1, 3)
    want = np.asarray(Image.fromarray(img, "RGB").convert("L")) != 0
    got = E.mask_of(np.ascontiguousarray(img.transpose(2, 0, 1)), 1)
    assert np.array_equal(got, want)
    assert not E.mask_of(np.array([1, 0, 0], np.uint8).reshape(3, 1, 1), 1)[0, 0]
    assert E.mask_of(np.array([1, 0, 0], np.uint8).reshape(3, 1, 1), 0)[0, 0]


def test_best_of_is_the_references_rule():
    from ctrlv_amd import metrics
    for name, (counts, want) in E.BEST_CASES.items():
        assert metrics.best_of(counts) == want, name
        assert metrics.best_of(np.array(counts, dtype=np.int64)) == want, name
        assert metrics.best_of(torch.tensor(counts, dtype=torch.int64)) == want, name
    # the reference's loop, literally
    for name, (counts, want) in E.BEST_CASES.items():
        best_score, best = -1, None
        for c, cand in enumerate(counts):
            gt, pred, inter = cand[0][0]
            miou = np.float64(inter) / np.float64(gt + pred - inter) if gt + pred - inter > 0 else 1
            best_score = max(best_score, miou)
            if best_score == miou:
                best = c
        assert [best] == want, name
    # two clips choose on their own
    two = [[a[0], b[0]] for a, b in zip(E.BEST_CASES["middle"][0], E.BEST_CASES["all_unions_zero"][0])]
    assert metrics.best_of(two) == [1, 2]
    scores = metrics.candidate_scores([[[[10, 20, 5], [4, 0, 0]]]])
    assert scores == [[((5 / 25, 5 / 20, 5 / 10), (0.0, 1, 0.0))]]


def test_pt_frames_to_u8_is_the_scripts_preparation():
    from ctrlv_amd import metrics
    f = torch.tensor([0.0, 4 / 255, 0.0196, 5 / 255, 0.5, 1.0])
    assert metrics.pt_frames_to_u8(f).tolist() == [0, 0, 0, 5, 127, 255]
    assert metrics.pt_frames_to_u8(f.to(torch.bfloat16)).dtype == torch.uint8
