"""The kernels between the box predictor and Box2Video on the device (include/ctrlv_hip.h: ctrlv_box_frames_post,
ctrlv_mask_counts; csrc/box_frames.hip) against tests/golden/box_chain_vectors.npz, which holds what the reference's own
statements (tools/eval_overall.py:96-105, src/ctrlv/metrics/FandJ.py:11-23) gave on seeded inputs.

The kernel forms y = clamp(x / 2 + 0.5, 0, 1) itself, so a golden y is fed as x = 2 y - 1.  The cases "grid", "grid_rolled" and
"pair" hold multiples of 1 / 256 only: x and the way back are exact in bf16 and fp16 (asserted), and out_u8 is compared with the
reference's recorded bytes.  "odd" holds arbitrary fp32 values: there y is what torch gives, operation by operation, in the
element type, and the expectation is tests/box_chain_utils.cleanup_numpy of that y -- pinned to the reference's bytes on every
golden input by tests/test_box_chain_cpu.py.  out_pt / out_cond are compared bit for bit with the torch expressions.

Every tensor lives in a guard-banded buffer (tests/guarded.py): inputs in NaN poison (0x7F bytes for uint8: a stray read counts
as a mask pixel), outputs in sentinels that must survive everywhere outside the view.  16 x 24 and 8 x 8 planes take the
16-pixel vector kernels, 7 x 13 the one-pixel ones."""
import numpy as np
import pytest
import torch

from tests import box_chain_utils as B
from tests import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = {"pt": ("pt",), "cond": ("cond",), "u8": ("u8",), "all": ("pt", "cond", "u8")}


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def el(request, hip_lib):
    return request.param


def _bits(t):
    return GD.as_int(t.contiguous())


def _guarded_input(data, fill="poison"):
    buf, flat = GD.guarded_flat(data.numel(), data.dtype, DEV, fill=fill)
    GD.put(flat, data.reshape(-1))
    return flat.view(data.shape)


def _case(names, el):
    """x (n F, 3, H, W) on the device, the torch y / cond of it, the expected bytes (n, F, 3, H, W), and F."""
    xs, wants = [], []
    for name in names:
        y_g = torch.from_numpy(B.G[name + "_y"])
        x = (2 * y_g - 1).to(el)
        y = (x.to(DEV) / 2 + 0.5).clamp(0, 1)
        exact = torch.equal(y.float().cpu(), y_g)
        assert exact == (name != "odd"), (name, el)
        wants.append(B.G[name + "_u8"] if exact else B.cleanup_numpy(y.float().cpu().numpy()))
        xs.append(x)
    x = _guarded_input(torch.cat(xs))
    y = (x / 2 + 0.5).clamp(0, 1)                 # tensor2vid(..., "pt"): every operation rounded to the element type
    return x, y, 2 * (y - 0.5), np.stack(wants), xs[0].shape[0]


def _run(x, F, which):
    from ctrlv_amd import ops
    m, _, H, W = x.shape
    shapes = {"pt": ((m, 3, H, W), x.dtype), "cond": ((m, 3, H, W), x.dtype), "u8": ((m // F, F, 3, H, W), torch.uint8)}
    bufs, args = {}, {}
    for name in ("pt", "cond", "u8"):
        if name in which:
            shape, dtype = shapes[name]
            buf, flat = GD.guarded_flat(int(np.prod(shape)), dtype, DEV)
            bufs[name] = (buf, buf.clone(), flat)
            args[name] = flat.view(shape)
        else:
            args[name] = False
    got = ops.box_frames_post(x, F, B.THRESHOLD, **args)
    torch.cuda.synchronize()
    return dict(zip(("pt", "cond", "u8"), got)), bufs


@pytest.mark.parametrize("which", list(OUTPUTS))
@pytest.mark.parametrize("names", [("grid",), ("odd",), ("pair",), ("grid", "grid_rolled"), ("odd", "odd")],
                         ids=lambda v: "+".join(v))
def test_box_frames_post_against_the_references_bytes(el, names, which):
    x, y, cond, want_u8, F = _case(names, el)
    got, bufs = _run(x, F, OUTPUTS[which])
    for name in ("pt", "cond", "u8"):
        if name not in OUTPUTS[which]:
            assert got[name] is None
    if "pt" in got and got["pt"] is not None:
        assert torch.equal(_bits(got["pt"]), _bits(y)), float((got["pt"].float() - y.float()).abs().max())
    if got["cond"] is not None:
        assert torch.equal(_bits(got["cond"]), _bits(cond)), float((got["cond"].float() - cond.float()).abs().max())
    if got["u8"] is not None:
        u8 = got["u8"].cpu().numpy()
        assert u8.shape == want_u8.shape
        bad = np.argwhere(u8 != want_u8)
        assert bad.size == 0, (len(bad), bad[:4].tolist())
    for name, (buf, before, flat) in bufs.items():
        expected = torch.from_numpy(want_u8).reshape(1, -1) if name == "u8" else None
        GD.check_written_only_inside(before, buf, flat.view(1, -1), expected=expected, what="out_" + name)


def test_the_frame_rule_is_per_clip_and_the_round_trip_is_not_the_identity(el):
    """Two clips of the same five frames, the second rotated by one: frame 1 of the first is blanked, in the second the same
    picture is frame 0 and stays, and the last picture, now frame 3, goes.  And cond is not x again in fp16."""
    x, y, cond, want_u8, F = _case(("grid", "grid_rolled"), el)
    got, _ = _run(x, F, ("cond", "u8"))
    u8 = got["u8"]
    assert not bool(u8[0, 1].any()) and bool(u8[1, 0].any())
    assert not bool(u8[1, 3].any()) and bool(u8[0, 4].any()) and bool(u8[1, 4].any())
    if el == torch.float16:           # x near 0 is finer than y near 0.5: 2 * (y - 0.5) cannot give every x back
        xo, _, _, _, Fo = _case(("odd",), el)
        back = _run(xo, Fo, ("cond",))[0]["cond"]
        assert not torch.equal(_bits(back), _bits(xo))


@pytest.mark.parametrize("names", [(n,) for n in B.IOU_CASES] + [("grid", "grid_rolled")], ids=lambda v: "+".join(v))
def test_mask_counts_and_the_metric_against_the_references(hip_lib, names):
    from ctrlv_amd import metrics, ops
    gt = _guarded_input(torch.from_numpy(np.stack([B.G[f"iou_{n}_gt"] for n in names])))
    pred = _guarded_input(torch.from_numpy(np.stack([B.G[f"iou_{n}_pred"] for n in names])))
    want = np.stack([B.G[f"iou_{n}_counts"] for n in names])
    buf, flat = GD.guarded_flat(len(names) * 6 * 8, torch.uint8, DEV)
    before = buf.clone()
    out = ops.mask_counts(gt, pred, out=flat.view(torch.int64).view(len(names), 2, 3))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want), (out.cpu().numpy().tolist(), want.tolist())
    GD.check_written_only_inside(before, buf, flat.view(1, -1), expected=torch.from_numpy(want).view(torch.uint8).reshape(1, -1),
                                 what="counts")
    for first_last, key in ((False, "all"), (True, "first_last")):
        got = metrics.binary_mask_iou(gt, pred, first_last=first_last)
        assert [tuple(t) for t in got] == [tuple(B.G[f"iou_{n}_{key}"]) for n in names], (key, got)
    one = metrics.binary_mask_iou(gt[0], pred[0])
    assert tuple(one) == tuple(B.G[f"iou_{names[0]}_all"])
