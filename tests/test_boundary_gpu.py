"""ctrlv_boundary_counts on the device (include/ctrlv_hip.h; csrc/box_eval.hip): the four counts of f_measure per frame, EXACTLY
those of the numpy restatement in tests/box_eval_ref.py (itself pinned to known answers by tests/test_box_eval_cpu.py) -- both
mask rules, seeded blocky masks and the known rectangle cases, widths with a ragged last word (65, 70, 129), heights that span
several bands of rows, every radius from the formula's own to 32, empty masks, unaligned inputs (the single-byte path) and guard
bands around the counts."""
import numpy as np
import pytest
import torch

from tests import box_eval_ref as E
from tests import guarded as Gd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1, 1), (1, 2, 2, 65), (2, 3, 37, 70), (1, 1, 64, 64), (1, 2, 96, 129), (1, 1, 150, 200), (1, 1, 300, 512)]
EXPLICIT = (1, 3, 10, 32)


def _inputs(shape, seed):
    n, F, H, W = shape
    gt, pred = E.blocky_u8(seed, n, F, H, W), E.blocky_u8(seed + 1000, n, F, H, W)
    if (H, W) == (E.H0, E.W0):
        (ga, pa), (gb, pb) = ((E.rect(*q) for q in E.RECTS[k]) for k in ("A", "B"))
        gt[0, 0], pred[0, 0] = E.as_u8(ga), E.as_u8(pa)
        gt[0, 1], pred[0, 1] = E.as_u8(gb), E.as_u8(pb)
        gt[0, 2], pred[0, 2] = 0, E.as_u8(pa)         # an empty ground truth
        gt[1, 0], pred[1, 0] = E.as_u8(gb), 0         # an empty prediction
        gt[1, 1], pred[1, 1] = 0, 0                   # both empty
    return gt, pred


def _unaligned(t):
    """The same bytes one byte off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 32, dtype=torch.uint8, device=t.device)
    off = (-buf.data_ptr()) % 16 + 1
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 1 and out.is_contiguous()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_boundary_counts_are_the_restatements(hip_lib, shape):
    from ctrlv_amd import metrics, ops
    n, F, H, W = shape
    gt, pred = _inputs(shape, 7 * H + W)
    d_gt, d_pred = torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV)
    u_gt, u_pred = _unaligned(d_gt), _unaligned(d_pred)
    own = metrics.boundary_radius(H, W)
    assert own == E.radius(H, W)
    nbytes = n * F * 4 * 8
    for mode in (0, 1):
        for r in sorted(set(EXPLICIT + (own,))):
            want = E.boundary_counts(gt, pred, mode, r)
            buf, flat = Gd.guarded_flat(nbytes, torch.uint8, DEV)
            before = buf.clone()
            out = flat.view(torch.int64).view(n, F, 4)
            got = ops.boundary_counts(d_gt, d_pred, r, mode, out=out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            assert np.array_equal(got.cpu().numpy(), want), (shape, mode, r, got.cpu().tolist(), want.tolist())
            Gd.check_written_only_inside(before, buf, flat.view(1, nbytes), torch.from_numpy(want).view(torch.uint8).view(1, nbytes),
                                         what=f"counts {shape} mode {mode} r {r}")
            again = ops.boundary_counts(u_gt, u_pred, r, mode)                  # the single-byte path
            assert np.array_equal(again.cpu().numpy(), want), (shape, mode, r, "unaligned")
            if (H, W) == (E.H0, E.W0) and mode == 1:
                for f, case in enumerate(("A", "B")):
                    if (case, r) in E.KNOWN:
                        assert tuple(want[0, f]) == E.KNOWN[(case, r)]
                assert want[0, 2, 1] == 0 and want[0, 2, 0] > 0                 # empty ground truth
                assert want[1, 0, 0] == 0 and want[1, 0, 1] > 0                 # empty prediction
                assert tuple(want[1, 1]) == (0, 0, 0, 0)
    if W > 1:
        assert E.boundary_counts(gt, pred, 0, own).sum() > 0                    # the masks are not all empty
    if shape == (2, 3, 37, 70):                                                 # the two mask rules see different masks
        assert not np.array_equal(E.boundary_counts(gt, pred, 0, own), E.boundary_counts(gt, pred, 1, own))


def test_boundary_f_measure_from_frames(hip_lib):
    """metrics.boundary_f_measure: (n, F) doubles from the device counts; the known F of case A at the radii 1 and 2."""
    from ctrlv_amd import metrics
    G, P = (E.rect(*q) for q in E.RECTS["A"])
    gt = torch.from_numpy(np.stack([E.as_u8(G), E.as_u8(G), np.zeros((3, E.H0, E.W0), np.uint8)])[None]).to(DEV)
    pred = torch.from_numpy(np.stack([E.as_u8(P), E.as_u8(G), np.zeros((3, E.H0, E.W0), np.uint8)])[None]).to(DEV)
    f1 = metrics.boundary_f_measure(gt, pred)                      # 37 x 70: radius 1
    assert f1.shape == (1, 3) and f1.dtype == np.float64
    assert f1[0, 0] == pytest.approx(E.KNOWN_F[("A", 1)], rel=0, abs=1e-15) and f1[0, 1:].tolist() == [1.0, 1.0]
    f2 = metrics.boundary_f_measure(gt[0], pred[0], mask="any", bound_th=2)
    assert f2.shape == (3,) and f2[0] == pytest.approx(E.KNOWN_F[("A", 2)], rel=0, abs=1e-15)
    with pytest.raises(ValueError, match="mask"):
        metrics.boundary_f_measure(gt, pred, mask="red")
