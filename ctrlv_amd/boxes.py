"""Box tables: the device records `ctrlv_render_box_frames` draws from (include/ctrlv_hip.h: ctrlv_box_object,
ctrlv_box_frame), built from the reference's label dicts (src/ctrlv/utils/plotting.py:33-124 reads `bbox`, `trackID`, `id_type`
and, with a camera matrix, `location`, `dimensions`, `rotation_y` / `alpha`).  The colours and the corner projection are the
library's host helpers, so a table built here equals one a foreign host builds through the C header."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import BOX_FILL, BOX_OUTLINE, BOX_WIRE, check

OBJECT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("fill_rgb", "u1", (4,)), ("line_rgb", "u1", (4,)),
                         ("corner", "<i2", (8, 2)), ("flags", "<u4"), ("reserved", "<i4")])
FRAME_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("kind", "<i4"), ("reserved", "<i4")])
assert OBJECT_DTYPE.itemsize == 64 and FRAME_DTYPE.itemsize == 16
KIND_BOX, KIND_TRAJECTORY = 0, 1
_I32 = 2 ** 31 - 1


def class_color(id_type):
    """ctrlv_box_class_color: the reference's class palette entry as it stands."""
    rgb = (ctypes.c_uint8 * 3)()
    check(_lib.load().ctrlv_box_class_color(int(id_type), rgb), "ctrlv_box_class_color")
    return tuple(rgb)


def track_color(seed, track_id):
    """ctrlv_box_track_color: a track's colour in [50, 254]^3 as a function of (seed, track_id)."""
    rgb = (ctypes.c_uint8 * 3)()
    check(_lib.load().ctrlv_box_track_color(int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id), rgb), "ctrlv_box_track_color")
    return tuple(rgb)


def project_corners(cam_to_img, location, dimensions, rot_y):
    """ctrlv_box_project_corners: the eight projected corners, int16 (8, 2), truncated and clamped to +-8191."""
    cam = np.ascontiguousarray(np.asarray(cam_to_img, dtype=np.float64))
    if cam.ndim != 2 or cam.shape[0] != 3:
        raise ValueError(f"project_corners: cam_to_img {cam.shape} must be (3, 3) or (3, 4)")
    loc = (ctypes.c_double * 3)(*[float(v) for v in location])
    dim = (ctypes.c_double * 3)(*[float(v) for v in dimensions])
    out = (ctypes.c_int16 * 16)()
    check(_lib.load().ctrlv_box_project_corners(cam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cam.shape[1], loc, dim,
                                                float(rot_y), out), "ctrlv_box_project_corners")
    return np.frombuffer(out, dtype=np.int16).reshape(8, 2).copy()


def _trunc(v):
    """The reference's int(...) on a float, kept inside int32 (the kernel clamps to +-8191)."""
    return max(-_I32, min(_I32, int(v)))


class BoxTable:
    """The two tables of n_clips x num_frames frames: `objects` uint8 (n_objects, 64) and `frames` int32 (n_clips * num_frames, 4),
    as tensors (`.to(device)` moves both)."""

    def __init__(self, objects, frames, n_clips, num_frames):
        self.objects, self.frames, self.n_clips, self.num_frames = objects, frames, int(n_clips), int(num_frames)
        if objects.dtype != torch.uint8 or objects.dim() != 2 or objects.shape[1] != 64 or objects.shape[0] < 1:
            raise ValueError("BoxTable: objects must be uint8 (n_objects >= 1, 64)")
        if frames.dtype != torch.int32 or tuple(frames.shape) != (self.n_clips * self.num_frames, 4):
            raise ValueError(f"BoxTable: frames must be int32 ({self.n_clips * self.num_frames}, 4)")

    @property
    def n_objects(self):
        return self.objects.shape[0]

    @property
    def n_frames(self):
        return self.frames.shape[0]

    @property
    def device(self):
        return self.objects.device

    def to(self, device):
        return BoxTable(self.objects.to(device).contiguous(), self.frames.to(device).contiguous(), self.n_clips, self.num_frames)

    def clip(self, i):
        """The table of clip i alone (the same object records; its frames' records)."""
        F = self.num_frames
        return BoxTable(self.objects, self.frames[i * F:(i + 1) * F].contiguous(), 1, F)

    @classmethod
    def from_records(cls, objects, frames, n_clips, num_frames):
        """From numpy structured arrays of OBJECT_DTYPE / FRAME_DTYPE (an empty object table gets one record that draws nothing)."""
        objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE).reshape(-1)
        if objects.size == 0:
            objects = np.zeros(1, dtype=OBJECT_DTYPE)
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE).reshape(-1)
        return cls(torch.from_numpy(objects.view(np.uint8).reshape(-1, 64).copy()),
                   torch.from_numpy(frames.view(np.int32).reshape(-1, 4).copy()), n_clips, num_frames)

    @classmethod
    def from_labels(cls, clips, cam_to_img=None, seed=0, is_gt=True, trajectory_last=False):
        """clips: per clip, per frame, a list of the reference's label dicts.  Every object is FILLed with its track's colour
        (`track_color(seed, trackID)`); without a camera matrix it gets the 2-D OUTLINE in its class colour, with one -- (3, 3)
        or (3, 4), or one per clip -- the projected WIRE instead, as plot_3d_bbox draws (rot_y = rotation_y when is_gt, else
        alpha / 180 * pi + arctan(x / z)).  trajectory_last: the last frame of every clip is a trajectory frame, its discs centred
        at (int((x1 + x2) / 2), int((y1 + y2) / 2)) on the floats (plot_trajectory)."""
        n = len(clips)
        if n < 1 or any(len(c) != len(clips[0]) for c in clips) or len(clips[0]) < 1:
            raise ValueError("BoxTable.from_labels: clips must be a non-empty list of clips of one length")
        F = len(clips[0])
        per_clip_cam = isinstance(cam_to_img, (list, tuple)) and np.asarray(cam_to_img[0]).ndim == 2
        objs, frames = [], np.zeros(n * F, dtype=FRAME_DTYPE)
        for ci, clip in enumerate(clips):
            cam = None if cam_to_img is None else (cam_to_img[ci] if per_clip_cam else cam_to_img)
            for fi, labels in enumerate(clip):
                traj = bool(trajectory_last) and fi == F - 1
                frames[ci * F + fi] = (len(objs), len(labels), KIND_TRAJECTORY if traj else KIND_BOX, 0)
                for lab in labels:
                    o = np.zeros((), dtype=OBJECT_DTYPE)
                    x1, y1, x2, y2 = [float(v) for v in lab["bbox"]]
                    o["x1"], o["y1"], o["x2"], o["y2"] = _trunc(x1), _trunc(y1), _trunc(x2), _trunc(y2)
                    o["fill_rgb"][:3] = track_color(seed, lab["trackID"])
                    o["line_rgb"][:3] = class_color(lab["id_type"])
                    if traj:
                        o["corner"][0] = (max(-8191, min(8191, int((x1 + x2) / 2))), max(-8191, min(8191, int((y1 + y2) / 2))))
                    elif cam is not None:
                        loc = lab["location"]
                        rot_y = lab["rotation_y"] if is_gt else lab["alpha"] / 180 * math.pi + math.atan(loc[0] / loc[2])
                        o["corner"] = project_corners(cam, loc, lab["dimensions"], rot_y)
                    o["flags"] = BOX_FILL | (BOX_OUTLINE if cam is None else BOX_WIRE)
                    objs.append(o)
        objects = np.array(objs, dtype=OBJECT_DTYPE) if objs else np.zeros(0, dtype=OBJECT_DTYPE)
        return cls.from_records(objects, frames, n, F)
