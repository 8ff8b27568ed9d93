"""Guard-banded tensors for the pitched-view tests (tests/test_pitched_gpu.py; proven on CPU tensors by
tests/test_guarded_cpu.py).  A helper module, not a conftest.

`guarded` places a [rows, cols] view inside a larger buffer the test owns: `pad_rows` whole rows in front and behind, a row
pitch wider than the view and a column offset, so that a kernel that mixes up a pitch with a width, walks past the ragged
edge of a tile or reads a conv halo it should have masked lands in memory whose every byte is known:

  fill = "poison"    inputs: every element of the buffer is a NaN of the tensor's type (e4m3 codes held as uint8: 0x7F) --
                     one stray read poisons the result it reaches;
  fill = "sentinel"  outputs: a NaN with a distinctive payload (uint8: the byte 0xA5) -- `check_written_only_inside` then
                     demands that no byte outside the view changed and no sentinel is left inside it.

Comparisons go through an integer reinterpretation of the bytes: NaN != NaN would hide exactly what is looked for."""
import torch

ROW_TILE = 256          # the tallest row tile of any kernel in csrc/
MIN_GAP = 64            # columns of gap a guarded buffer has at the least (left + right of the view)

# bit patterns of the fills, per element size: (poison, sentinel)
_FILLS = {
    torch.bfloat16: (0x7FC0, 0x7FE5),            # quiet NaN | quiet NaN, payload 0x25
    torch.float16: (0x7E00, 0x7EA5),             # quiet NaN | quiet NaN, payload 0xA5
    torch.float32: (0x7FC00000, 0x7FC0A5A5),
    torch.uint8: (0x7F, 0xA5),                   # the e4m3 NaN code | the byte the issue of this suite names
    torch.float8_e5m2: (0x7F, 0x7E),             # the lo plane of a split trunk tensor: two of e5m2's NaN codes
}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def guard_rows(W=0):
    """Rows of guard in front of and behind a view: one row tile plus the 3x3 conv halo of an image W pixels wide."""
    return ROW_TILE + W + 1


def as_int(t):
    """The same bytes as integers of the element's size (bit-exact comparisons; NaN payloads count)."""
    return t if t.dtype == torch.uint8 else t.view(_INT[t.element_size()])


def _signed(bits, nbytes):
    return bits - (1 << (8 * nbytes)) if nbytes > 1 and bits >= 1 << (8 * nbytes - 1) else bits


def fill_bits(dtype, fill):
    return _FILLS[dtype][{"poison": 0, "sentinel": 1}[fill]]


def fill_(t, fill):
    """Fill a contiguous tensor with the poison / sentinel pattern of its type, in place."""
    as_int(t).fill_(_signed(fill_bits(t.dtype, fill), t.element_size()))
    return t


def guarded(rows, cols, dtype, device, *, pitch=None, col_off=0, pad_rows=None, fill="sentinel"):
    """(buf, view): buf [pad_rows + rows + pad_rows, pitch] filled with `fill`, view = buf[pad_rows:pad_rows + rows,
    col_off:col_off + cols].  pitch = None: a dense operand (pitch = cols, col_off = 0), row guards only."""
    if pitch is None:
        pitch = cols
    if pad_rows is None:
        pad_rows = guard_rows()
    if col_off < 0 or col_off + cols > pitch or pad_rows < 0:
        raise ValueError(f"guarded: columns [{col_off}, {col_off + cols}) do not fit a pitch of {pitch}")
    buf = torch.empty(2 * pad_rows + rows, pitch, dtype=dtype, device=device)
    as_int(buf).fill_(_signed(fill_bits(dtype, fill), buf.element_size()))
    return buf, buf[pad_rows:pad_rows + rows, col_off:col_off + cols]


def guarded_flat(numel, dtype, device, *, fill="sentinel", gap=MIN_GAP):
    """(buf, flat): a contiguous run of `numel` elements (a dense tensor of any shape: flat.view(shape)) with `gap` elements
    of guard on either side inside its row and one row of guard above and below; check it through flat.view(1, numel)."""
    pitch = (numel + 2 * gap + 63) // 64 * 64          # (rows of the buffer keep the 64-element alignment of its base)
    buf, view = guarded(1, numel, dtype, device, pitch=pitch, col_off=gap, pad_rows=1, fill=fill)
    return buf, view[0]


def put(view, data):
    """Copy host data into a guarded view (same shape; the buffer around it keeps its fill)."""
    if tuple(view.shape) != tuple(data.shape):
        raise ValueError(f"put: view {tuple(view.shape)} and data {tuple(data.shape)} differ")
    view.copy_(data.to(view.dtype))
    return view


def _place(buf, view):
    if (view.dim() != 2 or buf.dim() != 2 or view.stride(1) != 1 or view.dtype != buf.dtype
            or (view.shape[0] > 1 and view.stride(0) != buf.stride(0))):
        raise ValueError("check_written_only_inside: view must be a 2-D column / row slice of buf")
    off = view.storage_offset() - buf.storage_offset()
    r0, c0 = divmod(off, buf.stride(0))
    if off < 0 or r0 + view.shape[0] > buf.shape[0] or c0 + view.shape[1] > buf.shape[1]:
        raise ValueError("check_written_only_inside: view does not lie inside buf")
    return r0, c0


def check_written_only_inside(buf_before, buf, view, expected=None, what="output"):
    """Assert that (1) every byte of `buf` outside `view` is bit-identical to `buf_before` (a clone taken before the
    launch) and (2) every element inside `view` was written: finite for a float type; for the byte planes (uint8 codes,
    e5m2 lo planes), whose every code is a legal value, no element still holds the sentinel unless `expected` (the dense
    result of the same launch) holds that very byte there.  A failure names the region that was hit -- rows before, rows
    after, left gap, right gap -- and the first offending (row, col) of `buf`."""
    r0, c0 = _place(buf, view)
    rows, cols = view.shape
    changed = as_int(buf) != as_int(buf_before)
    changed[r0:r0 + rows, c0:c0 + cols] = False
    if bool(changed.any()):
        r, c = (int(v) for v in changed.nonzero()[0])
        region = ("rows before" if r < r0 else "rows after" if r >= r0 + rows else "left gap" if c < c0 else "right gap")
        raise AssertionError(f"{what}: {int(changed.sum())} element(s) written outside the view, first in the {region} at "
                             f"(row {r}, col {c}) of the buffer; view = rows [{r0}, {r0 + rows}) x cols [{c0}, {c0 + cols})")
    if view.dtype in (torch.uint8, torch.float8_e5m2):
        left = as_int(view) == fill_bits(view.dtype, "sentinel")
        if expected is not None:
            left &= as_int(expected.to(view.device)) != fill_bits(view.dtype, "sentinel")
    else:
        left = ~torch.isfinite(view)
    if bool(left.any()):
        r, c = (int(v) for v in left.nonzero()[0])
        raise AssertionError(f"{what}: {int(left.sum())} element(s) inside the view not written (or not finite), first at "
                             f"(row {r}, col {c}) of the view")
