"""numpy restatement of the section "Box and trajectory frames from coordinates" of include/ctrlv_hip.h: the integer picture
(capsules, rect / ring / wire, the three layers and their blend, the trajectory discs), the safety rules of the two tables, and the
host helpers (class palette, track colour on tests/seeded_ref.py's Philox, corner projection).  A helper module, not a conftest:
tests/test_box_render_cpu.py proves the restatement (PIL's filled rectangles, a hand-written ring, the blend table) and holds the
C helpers against it, tests/test_box_render_gpu.py holds the kernels against it.  Everything is int64; nothing here is OpenCV."""
import numpy as np

from tests import seeded_ref as S

OBJECT_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("fill_rgb", "u1", (4,)), ("line_rgb", "u1", (4,)),
                         ("corner", "<i2", (8, 2)), ("flags", "<u4"), ("reserved", "<i4")])
FRAME_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("kind", "<i4"), ("reserved", "<i4")])
FILL, OUTLINE, WIRE = 1, 2, 4
CLAMP, MAX_COUNT = 8191, 1024
# plotting.py:30 TYPE_LOOKUP, the numbers as they stand there
PALETTE = [(255, 0, 0), (255, 255, 255), (0, 0, 255), (2, 255, 250), (247, 44, 200), (42, 42, 165), (0, 255, 0), (44, 162, 247),
           (255, 153, 204), (204, 204, 255), (128, 128, 128)]
WIRE_EDGES = [(2 * i, 2 * i + 1, 4) for i in range(4)] + [(i, (i + 2) % 8, 4) for i in range(8)] + [(2, 5, 1), (3, 4, 1)]


def obj(x1=0, y1=0, x2=0, y2=0, fill=(0, 0, 0), line=(0, 0, 0), corner=None, flags=0):
    o = np.zeros((), dtype=OBJECT_DTYPE)
    o["x1"], o["y1"], o["x2"], o["y2"] = x1, y1, x2, y2
    o["fill_rgb"][:3], o["line_rgb"][:3] = fill, line
    if corner is not None:
        c = np.zeros((8, 2), dtype=np.int16)
        c[:len(corner)] = corner
        o["corner"] = c
    o["flags"] = flags
    return o


def tables(frames_of_objects, kinds=None):
    """A list (per frame) of lists of objects -> (objects, frames) structured arrays, the frames in order."""
    objs, fr = [], np.zeros(len(frames_of_objects), dtype=FRAME_DTYPE)
    for j, lst in enumerate(frames_of_objects):
        fr[j] = (len(objs), len(lst), 0 if kinds is None else kinds[j], 0)
        objs += lst
    return (np.array(objs, dtype=OBJECT_DTYPE) if objs else np.zeros(1, dtype=OBJECT_DTYPE)), fr


def capsule(p0, p1, r4, X, Y):
    """The coverage mask of capsule(P0, P1, R4) on the int64 pixel grids X, Y."""
    dx, dy = int(p1[0]) - int(p0[0]), int(p1[1]) - int(p0[1])
    ex, ey = X - int(p0[0]), Y - int(p0[1])
    L, t = dx * dx + dy * dy, dx * ex + dy * ey
    start = 4 * (ex * ex + ey * ey) <= r4
    fx, fy = X - int(p1[0]), Y - int(p1[1])
    end = 4 * (fx * fx + fy * fy) <= r4
    cr = dx * ey - dy * ex
    mid = 4 * cr * cr <= r4 * L
    if L == 0:
        return start
    return np.where(t <= 0, start, np.where(t >= L, end, mid))


def _clamp(v):
    return int(max(-CLAMP, min(CLAMP, int(v))))


def rect_mask(o, X, Y):
    x1, x2, y1, y2 = _clamp(o["x1"]), _clamp(o["x2"]), _clamp(o["y1"]), _clamp(o["y2"])
    return (X >= min(x1, x2)) & (X <= max(x1, x2)) & (Y >= min(y1, y2)) & (Y <= max(y1, y2))


def ring_mask(o, X, Y):
    x1, x2, y1, y2 = _clamp(o["x1"]), _clamp(o["x2"]), _clamp(o["y1"]), _clamp(o["y2"])
    xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    m = np.zeros(X.shape, dtype=bool)
    for p0, p1 in (((xa, ya), (xb, ya)), ((xb, ya), (xb, yb)), ((xb, yb), (xa, yb)), ((xa, yb), (xa, ya))):
        m |= capsule(p0, p1, 4, X, Y)
    return m


def wire_mask(o, X, Y):
    c = [(_clamp(o["corner"][i][0]), _clamp(o["corner"][i][1])) for i in range(8)]
    m = np.zeros(X.shape, dtype=bool)
    for a, b, r4 in WIRE_EDGES:
        m |= capsule(c[a], c[b], r4, X, Y)
    return m


def rhe_quarter(s):
    """round-half-to-even of s / 4 for non-negative integers."""
    q, r = s // 4, s % 4
    return q + np.where(r == 3, 1, np.where(r == 2, q & 1, 0))


def frame_objects(fr, n_objects):
    first, count = int(fr["first"]), int(fr["count"])
    if first < 0 or first >= n_objects:
        return range(0)
    return range(first, first + max(0, min(count, n_objects - first, MAX_COUNT)))


def render(objects, frames, Hs, Ws):
    """(n_frames, 3, Hs, Ws) uint8."""
    Y, X = np.meshgrid(np.arange(Hs, dtype=np.int64), np.arange(Ws, dtype=np.int64), indexing="ij")
    out = np.zeros((len(frames), 3, Hs, Ws), dtype=np.uint8)
    for j, fr in enumerate(frames):
        U, T, W = (np.zeros((3, Hs, Ws), dtype=np.int64) for _ in range(3))
        for i in frame_objects(fr, len(objects)):
            o = objects[i]
            fill, line = o["fill_rgb"][:3].astype(np.int64), o["line_rgb"][:3].astype(np.int64)
            if int(fr["kind"]) == 1:
                cx, cy = _clamp(o["corner"][0][0]), _clamp(o["corner"][0][1])
                d2 = (X - cx) ** 2 + (Y - cy) ** 2
                for r2, col in ((400, fill), (100, line)):
                    U = np.where((d2 <= r2)[None], col[:, None, None], U)
                continue
            flags = int(o["flags"])
            if flags & OUTLINE:
                U = np.where(ring_mask(o, X, Y)[None], line[:, None, None], U)
            if flags & FILL:
                T = np.where(rect_mask(o, X, Y)[None], fill[:, None, None], T)
            if flags & WIRE:
                W = np.where(wire_mask(o, X, Y)[None], line[:, None, None], W)
        out[j] = np.where(W != 0, W, np.where(T != 0, rhe_quarter(3 * T + U), U)).astype(np.uint8)
    return out


def track_color(seed, track_id):
    seed, t = int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id) & 0xFFFFFFFFFFFFFFFF
    one = lambda v: np.array([v], dtype=np.uint64)      # noqa: E731
    x = S.philox4x32_10((one(t & 0xFFFFFFFF), one(t >> 32), one(7), one(0)), (seed & 0xFFFFFFFF, seed >> 32))
    return tuple(50 + ((int(x[c][0]) * 205) >> 32) for c in range(3))


def project_corners_float(cam_to_img, location, dimensions, rot_y):
    """The eight projected corners before truncation, float64 (8, 2), as plotting.py:81-93 computes them."""
    cam = np.asarray(cam_to_img, dtype=np.float64)
    center, dims = np.asarray(location, dtype=np.float64), np.asarray(dimensions, dtype=np.float64)
    pts = []
    for i in (1, -1):
        for j in (1, -1):
            for k in (0, 1):
                point = np.copy(center)
                point[0] = center[0] + i * dims[1] / 2 * np.cos(-rot_y + np.pi / 2) + (j * i) * dims[2] / 2 * np.cos(-rot_y)
                point[2] = center[2] + i * dims[1] / 2 * np.sin(-rot_y + np.pi / 2) + (j * i) * dims[2] / 2 * np.sin(-rot_y)
                point[1] = center[1] - k * dims[0]
                if cam.shape[1] == 4:
                    point = np.append(point, 1)
                v = [sum(float(cam[r, c]) * float(point[c]) for c in range(cam.shape[1])) for r in range(3)]   # in column order
                den = v[2] if abs(v[2]) > 1e-4 else 1e-4
                pts.append((v[0] / den, v[1] / den))
    return np.array(pts, dtype=np.float64)


def project_corners(cam_to_img, location, dimensions, rot_y):
    u = project_corners_float(cam_to_img, location, dimensions, rot_y)
    return np.clip(np.trunc(np.nan_to_num(u, nan=0.0, posinf=CLAMP, neginf=-CLAMP)), -CLAMP, CLAMP).astype(np.int16)
