"""tests/guarded.py on CPU tensors (no GPU): the checker behind tests/test_pitched_gpu.py fires for a write in each of the
four regions outside a view and for an element of the view left unwritten, compares bits (an overwrite with the same value
is no write; a NaN of another payload is), and passes a correct in-view write."""
import pytest
import torch

from tests.guarded import as_int, check_written_only_inside, fill_bits, guard_rows, guarded, guarded_flat, put

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.float8_e5m2]
IDS = ["bf16", "fp16", "fp32", "u8", "e5m2"]
ROWS, COLS, PITCH, OFF, PAD = 5, 12, 12 + 64, 24, 3


def _data(dtype, rows=ROWS, cols=COLS):
    x = torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) % 7 + 1
    return x.to(torch.uint8) if dtype == torch.uint8 else x.to(dtype)


def _fresh(dtype, fill="sentinel"):
    buf, view = guarded(ROWS, COLS, dtype, "cpu", pitch=PITCH, col_off=OFF, pad_rows=PAD, fill=fill)
    return buf, view, buf.clone()


def _poke(buf, r, c, bits):
    as_int(buf)[r, c] = bits


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_and_fills(dtype):
    for fill in ("poison", "sentinel"):
        buf, view, _ = _fresh(dtype, fill)
        assert tuple(buf.shape) == (PAD + ROWS + PAD, PITCH) and tuple(view.shape) == (ROWS, COLS)
        assert view.data_ptr() == buf.data_ptr() + (PAD * PITCH + OFF) * buf.element_size()
        assert view.stride(0) == PITCH and view.stride(1) == 1
        bits = fill_bits(dtype, fill)
        assert bool((as_int(buf).to(torch.int64) & ((1 << 8 * buf.element_size()) - 1) == bits).all())
        if dtype != torch.uint8:
            assert bool(torch.isnan(buf.float()).all()), "the fills of a float type are NaNs"
    assert fill_bits(dtype, "poison") != fill_bits(dtype, "sentinel")
    assert fill_bits(torch.uint8, "poison") == 0x7F and fill_bits(torch.uint8, "sentinel") == 0xA5
    # dense operands keep the row guards; the default guard is a row tile plus the conv halo
    buf, view = guarded(4, 8, dtype, "cpu")
    assert buf.shape[1] == 8 and view.is_contiguous() and buf.shape[0] == 4 + 2 * guard_rows() and guard_rows(64) == 256 + 64 + 1
    with pytest.raises(ValueError):
        guarded(4, 8, dtype, "cpu", pitch=12, col_off=8)
    fb, flat = guarded_flat(10, dtype, "cpu")
    assert flat.is_contiguous() and flat.numel() == 10 and fb.shape == (3, 192) and flat.storage_offset() == 192 + 64


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_correct_write_passes(dtype):
    buf, view, before = _fresh(dtype)
    put(view, _data(dtype))
    check_written_only_inside(before, buf, view)
    assert torch.equal(as_int(view), as_int(_data(dtype)))
    fb, flat = guarded_flat(10, dtype, "cpu")
    fbefore = fb.clone()
    put(flat, _data(dtype, 1, 10)[0])
    check_written_only_inside(fbefore, fb, flat.view(1, 10))
    with pytest.raises(ValueError):
        put(view, _data(dtype)[:, :4])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("region,r,c", [("rows before", PAD - 1, OFF + 3), ("rows after", PAD + ROWS, OFF),
                                        ("left gap", PAD + 2, OFF - 1), ("right gap", PAD + ROWS - 1, OFF + COLS),
                                        ("rows before", 0, 0), ("rows after", 2 * PAD + ROWS - 1, PITCH - 1)])
def test_one_element_outside_fires(dtype, region, r, c):
    buf, view, before = _fresh(dtype)
    put(view, _data(dtype))
    _poke(buf, r, c, 1)
    with pytest.raises(AssertionError, match=rf"{region} at \(row {r}, col {c}\)"):
        check_written_only_inside(before, buf, view)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_unwritten_element_fires(dtype):
    buf, view, before = _fresh(dtype)
    data = _data(dtype)
    put(view, data)
    _poke(buf, PAD + 3, OFF + 7, as_int(before)[0, 0])            # (3, 7) of the view keeps the sentinel
    with pytest.raises(AssertionError, match=r"not written.*\(row 3, col 7\) of the view"):
        check_written_only_inside(before, buf, view)
    if dtype in (torch.uint8, torch.float8_e5m2):
        # a byte plane's every code is a value: where the dense result holds the sentinel byte itself, it is no leftover
        with pytest.raises(AssertionError, match="not written"):
            check_written_only_inside(before, buf, view, expected=data)
        want = data.clone()
        as_int(want)[3, 7] = as_int(before)[0, 0]
        check_written_only_inside(before, buf, view, expected=want)
    else:
        # any non-finite value inside the view fires, an infinity included
        put(view, data)
        view[1, 2] = float("inf")
        with pytest.raises(AssertionError, match=r"\(row 1, col 2\) of the view"):
            check_written_only_inside(before, buf, view)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_are_compared_not_values(dtype):
    buf, view, before = _fresh(dtype)
    put(view, _data(dtype))
    # an outside element overwritten with the very value it held: not a change (a float == would call NaN != NaN one)
    _poke(buf, 1, 5, as_int(before)[1, 5])
    buf[PAD + ROWS + 1, 2:9] = before[PAD + ROWS + 1, 2:9]
    check_written_only_inside(before, buf, view)
    # an outside NaN replaced by a NaN of another payload: a change, though both are NaN
    other = fill_bits(dtype, "poison")
    assert other != fill_bits(dtype, "sentinel")
    _poke(buf, PAD + 1, OFF + COLS + 2, other)
    if dtype != torch.uint8:
        assert bool(torch.isnan(buf[PAD + 1, OFF + COLS + 2].float()))
    with pytest.raises(AssertionError, match="right gap"):
        check_written_only_inside(before, buf, view)


def test_the_view_must_be_a_slice_of_the_buffer():
    buf, view, before = _fresh(torch.float32)
    with pytest.raises(ValueError):
        check_written_only_inside(before, buf, torch.zeros(ROWS, COLS))
    with pytest.raises(ValueError):
        check_written_only_inside(before, buf, view[:, ::2])
